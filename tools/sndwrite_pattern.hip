// sndwrite_pattern.hip — the memory pattern of the application write's copy
// (mtcp_amd/csrc/sndwrite_kernels.hpp) without plan, search and shift: the
// yardstick of tools/sndwrite_bench.py.  Measurement infrastructure: nothing
// here is part of libmtcp_gpu.so.
//
// The pattern: a wave per copy unit on the copy kernel's grid rule.  unit[u] =
// {source byte offset >> 4, destination byte offset >> 4, pieces, 0}, written by
// the host: the wave loads `pieces` aligned 16 B pieces of the source region,
// non-temporal, four a lane, all before the first store, and stores them to the
// arena's grid with plain stores.  No request lookup, no second source piece,
// no funnel shift, no partial store, no move: the pieces at a run's ends are
// stored whole, so it runs on an arena of its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mtcp_amd/csrc/sndwrite_kernels.hpp"

namespace {

using namespace mg;

__global__ __launch_bounds__(kBlock) void pattern_copy(const uint4 *__restrict__ unit, uint32_t units, uint64_t sbase,
                                                       uint64_t src_bytes, uint64_t arena, uint64_t arena_bytes) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + threadIdx.x / kWave));
    const uint32_t waves = gridDim.x * kWavesPerBlock;
    for (uint32_t u = wave; u < units; u += waves) {
        const uint4 r = unit[u];
        v4u v[kReadRounds];
#pragma unroll
        for (int k = 0; k < kReadRounds; ++k) {
            const uint32_t c = lane + (uint32_t)k * kWave;
            const uint64_t s = 16ull * ((uint64_t)r.x + c);
            v[k] = v4u{0u, 0u, 0u, 0u};
            if (c < r.z && s + 16 <= src_bytes) v[k] = gload_nt(sbase + s);
        }
#pragma unroll
        for (int k = 0; k < kReadRounds; ++k) {
            const uint32_t c = lane + (uint32_t)k * kWave;
            const uint64_t d = 16ull * ((uint64_t)r.y + c);
            if (c < r.z && d + 16 <= arena_bytes) *reinterpret_cast<gsv4u *>(arena + d) = v[k];
        }
    }
}

}  // namespace

extern "C" {

// grid: as mtcp_gpu_sndwrite_dev sizes its copy launch (cu8 = 8 workgroups per CU).
int sndwrite_pattern_dev(const void *d_unit, uint32_t units, const void *d_src, uint64_t src_bytes, void *d_arena,
                         uint64_t arena_bytes, uint32_t cu8, void *stream) {
    if (!units) return 0;
    const uint32_t wgs = (units + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(pattern_copy, dim3(wgs < cu8 ? wgs : cu8), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint4 *>(d_unit), units, reinterpret_cast<uint64_t>(d_src), src_bytes,
                       reinterpret_cast<uint64_t>(d_arena), arena_bytes);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // extern "C"
