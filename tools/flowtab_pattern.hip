// flowtab_pattern.hip — the yardsticks of tools/flowtab_bench.py.  Measurement
// infrastructure: nothing here is part of libmtcp_gpu.so.
//
//   flowtab_pattern_launch   the memory pattern of flowtab_lookup_kernel
//       (mtcp_amd/csrc/flowtab_kernels.hpp) without hashing, comparing and
//       probing: the same four record dwords per lane on the same grid, ONE
//       16 B gather per TCP_OK record at a pseudo-random slot that costs one
//       multiply of the record's index, and the same 4 B stores.
//   flowtab_lookup_group_launch   the product's lookup kernel itself with G
//       slots loaded per probe step (1, 2 or 4), on the product's grid: how
//       the library's choice of G was measured.
//   flowtab_cpu_walk   one host core walking a chained table over the same
//       records: 131 072 bins of singly linked items, HashFlow, first equal
//       key.  A restatement of mtcp/src/fhash.c:103-121 written for this tool,
//       for scale only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "../mtcp_amd/csrc/flowtab_kernels.hpp"

namespace {

constexpr uint32_t kBlock = 256;

__global__ __launch_bounds__(kBlock) void pattern_lookup(const mtcp_gpu_result *__restrict__ res, uint32_t n,
                                                         const uint4 *__restrict__ slots, uint32_t mask,
                                                         uint32_t *__restrict__ sid, uint32_t *__restrict__ bins) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const uint32_t *r = reinterpret_cast<const uint32_t *>(res + i);
        const uint32_t a = r[0], b = r[1], c = r[2], verdict = r[9] & 0xFFu;
        uint32_t out = 0xFFFFFFFFu;
        if (verdict == 0) {
            const uint4 v = slots[(i * 2654435761u >> 4) & mask];
            out = v.w ^ v.x;
        }
        sid[i] = out;
        if (bins) bins[i] = a ^ b ^ c;
    }
}

uint32_t product_grid(uint32_t n) {
    int dev = 0, cus = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return std::max(1u, std::min<uint32_t>((n + kBlock - 1) / kBlock, (uint32_t)cus * 8));
}

}  // namespace

extern "C" int flowtab_pattern_launch(const void *d_res, uint32_t n, const void *d_slots, uint32_t cap_log2,
                                      uint32_t *d_sid, uint32_t *d_bins, void *stream) {
    hipLaunchKernelGGL(pattern_lookup, dim3(product_grid(n)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       static_cast<const mtcp_gpu_result *>(d_res), n, static_cast<const uint4 *>(d_slots),
                       (1u << cap_log2) - 1, d_sid, d_bins);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// d_slots: a table image in the library's layout (the tool builds its own
// with the model's pairs through flowtab_build below).
extern "C" int flowtab_lookup_group_launch(int G, const void *d_res, uint32_t n, const void *d_slots,
                                           uint32_t cap_log2, uint32_t *d_sid, uint32_t *d_bins, void *stream) {
    const dim3 grid(product_grid(n)), block(kBlock);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const mtcp_gpu_result *res = static_cast<const mtcp_gpu_result *>(d_res);
    const uint4 *slots = static_cast<const uint4 *>(d_slots);
    const uint32_t mask = (1u << cap_log2) - 1;
    if (G == 1)
        hipLaunchKernelGGL(mg::flowtab_lookup_kernel<1>, grid, block, 0, st, res, n, slots, mask, d_sid, d_bins);
    else if (G == 2)
        hipLaunchKernelGGL(mg::flowtab_lookup_kernel<2>, grid, block, 0, st, res, n, slots, mask, d_sid, d_bins);
    else if (G == 4)
        hipLaunchKernelGGL(mg::flowtab_lookup_kernel<4>, grid, block, 0, st, res, n, slots, mask, d_sid, d_bins);
    else
        return -1;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// A table image for flowtab_lookup_group_launch: d_slots cleared to EMPTY,
// then the product's insert and remove kernels over the entries (d_stats: 16 B, zeroed here).
extern "C" int flowtab_build(void *d_slots, uint32_t cap_log2, const void *d_ins, uint32_t n_ins,
                             const void *d_del, uint32_t n_del, uint32_t *d_stats, void *stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t mask = (1u << cap_log2) - 1;
    if (hipMemsetAsync(d_slots, 0xFF, sizeof(uint4) << cap_log2, st) != hipSuccess ||
        hipMemsetAsync(d_stats, 0, 16, st) != hipSuccess)
        return -1;
    if (n_ins)
        hipLaunchKernelGGL(mg::flowtab_insert_kernel, dim3(product_grid(n_ins)), dim3(kBlock), 0, st,
                           static_cast<uint4 *>(d_slots), mask, static_cast<const uint4 *>(d_ins), n_ins, d_stats);
    if (n_del)
        hipLaunchKernelGGL(mg::flowtab_remove_kernel, dim3(product_grid(n_del)), dim3(kBlock), 0, st,
                           static_cast<uint4 *>(d_slots), mask, static_cast<const uint4 *>(d_del), n_del, d_stats);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// One host core: build the chained table from ent[0 .. n_ent) (append at the
// bin's tail), then `reps` timed walks over the n records; sid as the device
// writes it (first equal key: the entries carry no duplicate keys).  Returns
// the best walk in seconds.
extern "C" double flowtab_cpu_walk(const mtcp_gpu_result *res, uint32_t n, const mtcp_gpu_flow_entry *ent,
                                   uint32_t n_ent, uint32_t *sid, int reps) {
    constexpr uint32_t kBins = MTCP_GPU_NUM_BINS_FLOWS, kNil = 0xFFFFFFFFu;
    std::vector<uint32_t> head(kBins, kNil), tail(kBins, kNil), next(n_ent, kNil);
    auto bin_of = [](const uint32_t (&k)[3]) { return mg::hash_flow32(k) & (kBins - 1); };
    for (uint32_t i = 0; i < n_ent; ++i) {
        uint32_t k[3];
        memcpy(k, &ent[i], 12);
        const uint32_t b = bin_of(k);
        if (tail[b] == kNil) head[b] = i; else next[tail[b]] = i;
        tail[b] = i;
    }
    double best = -1;
    for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t i = 0; i < n; ++i) {
            if (res[i].verdict != MTCP_GPU_V_TCP_OK) {
                sid[i] = MTCP_GPU_FLOW_NONE;
                continue;
            }
            uint32_t k[3];
            memcpy(&k[0], &res[i].daddr, 4);
            memcpy(&k[1], &res[i].saddr, 4);
            k[2] = (uint32_t)res[i].dport | ((uint32_t)res[i].sport << 16);
            uint32_t found = MTCP_GPU_FLOW_MISS;
            for (uint32_t e = head[bin_of(k)]; e != kNil; e = next[e])
                if (memcmp(&ent[e], k, 12) == 0) {
                    found = ent[e].id;
                    break;
                }
            sid[i] = found;
        }
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (best < 0 || dt < best) best = dt;
    }
    return best;
}
