// txseg_pattern.hip — the yardstick of tools/txseg_bench.py (measurement only,
// not the product): the memory access pattern of the segment passes
// (mtcp_amd/csrc/txseg_kernels.hpp) without their arithmetic and without the
// search.  The same grids and the same traffic: plan loads 64 B per burst,
// parks 16 B per burst and writes one pair of sums per workgroup; scan reads
// and rewrites those pairs in one workgroup; place loads the parked 16 B and
// stores 4 + 8 B of workspace and a 16 B result per burst; emit stores 4 B of
// every result, stages its tile's bursts' 4 + 8 B of workspace in LDS, and per
// record loads its burst's 64 B and stores 48 B and an 8 B descriptor, four
// records per lane on the same 1 024-record tiles.  What differs: no
// validation, no divisions, no scans, no fetch-and-min, and record k's burst is
// k * n_burst / seg_cap (one multiply) instead of a search, so the bursts a
// tile reads are as contiguous as with an even fan-out.  The records it writes
// are not segment records; the tool never reads them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mtcp_amd/csrc/txseg_kernels.hpp"

namespace {

using namespace mg;

__device__ __forceinline__ v4u burst_words(const void *burst, uint32_t i, v4u &q1, v4u &q2, v4u &q3) {
    const uint64_t a = (uint64_t)burst + 64ull * i;
    q1 = gload(a + 16), q2 = gload(a + 32), q3 = gload(a + 48);
    return gload(a);
}

__global__ __launch_bounds__(kBlock) void pattern_plan(const void *__restrict__ burst, uint32_t n,
                                                       void *__restrict__ park, uint32_t *__restrict__ part_c,
                                                       uint64_t *__restrict__ part_b) {
    __shared__ uint32_t acc[kWavesPerBlock];
    const uint32_t i = blockIdx.x * kTxsegTile + threadIdx.x;
    uint32_t x = 0;
    if (i < n) {
        v4u q1, q2, q3;
        const v4u q0 = burst_words(burst, i, q1, q2, q3);
        const v4u v = q0 ^ q1 ^ q2 ^ q3;
        *reinterpret_cast<gsv4u *>((uint64_t)park + 16ull * i) = v;
        x = v.x ^ v.y ^ v.z ^ v.w;
    }
    if ((threadIdx.x & (kWave - 1)) == 0) acc[threadIdx.x / kWave] = x;
    __syncthreads();
    if (threadIdx.x == 0) part_c[blockIdx.x] = acc[0] ^ acc[1] ^ acc[2] ^ acc[3], part_b[blockIdx.x] = acc[0];
}

__global__ __launch_bounds__(kBlock) void pattern_scan(uint32_t *__restrict__ part_c, uint64_t *__restrict__ part_b,
                                                       uint32_t nwg, uint32_t *__restrict__ tot_c,
                                                       unsigned long long *__restrict__ tot_b) {
    uint32_t acc = 0;
    for (uint32_t i = threadIdx.x; i < nwg; i += kBlock) {
        const uint32_t c = part_c[i];
        const uint64_t b = part_b[i];
        part_c[i] = c + 1, part_b[i] = b + 1;
        acc += c + (uint32_t)b;
    }
    if (threadIdx.x == 0) *tot_c = acc, *tot_b = acc;
}

__global__ __launch_bounds__(kBlock) void pattern_place(const void *__restrict__ park, uint32_t n,
                                                        const uint32_t *__restrict__ part_c,
                                                        const uint64_t *__restrict__ part_b,
                                                        uint32_t *__restrict__ first, uint64_t *__restrict__ boff,
                                                        void *__restrict__ res) {
    const uint32_t i = blockIdx.x * kTxsegTile + threadIdx.x;
    if (i >= n) return;
    const v4u q = gload((uint64_t)park + 16ull * i);
    const uint32_t c = part_c[blockIdx.x];
    const uint64_t b = part_b[blockIdx.x];
    first[i] = c ^ q.x;
    boff[i] = b ^ q.y;
    const v4u r = {q.y, q.z, q.w, c};
    *reinterpret_cast<gsv4u *>((uint64_t)res + 16ull * i) = r;
}

__device__ __forceinline__ void pattern_record(const void *burst, uint32_t i, uint32_t f, uint64_t b, void *seg,
                                               void *desc, uint32_t k) {
    v4u q1, q2, q3;
    const v4u q0 = burst_words(burst, i, q1, q2, q3);
    const uint64_t at = (uint64_t)seg + 48ull * k;
    const v4u c = {q2.x ^ q3.x, q2.y ^ q3.y, q2.z ^ q3.z ^ f, q2.w ^ q3.w ^ k};
    *reinterpret_cast<gsv4u *>(at) = q0;
    *reinterpret_cast<gsv4u *>(at + 16) = q1;
    *reinterpret_cast<gsv4u *>(at + 32) = c;
    const v2u d = {(uint32_t)b, (uint32_t)(b >> 32) ^ k};
    *reinterpret_cast<gsv2u *>((uint64_t)desc + 8ull * k) = d;
}

__global__ __launch_bounds__(kBlock) void pattern_emit(const void *__restrict__ burst, uint32_t n, uint32_t seg_cap,
                                                       uint64_t ratio, const uint32_t *__restrict__ first,
                                                       const uint64_t *__restrict__ boff,
                                                       const uint32_t *__restrict__ tot_c,
                                                       const unsigned long long *__restrict__ tot_b,
                                                       void *__restrict__ seg, void *__restrict__ desc,
                                                       void *__restrict__ res, uint64_t *__restrict__ d_total) {
    const uint32_t T = *tot_c;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
        *reinterpret_cast<__attribute__((address_space(1))) uint32_t *>((uint64_t)res + 16ull * i) = first[i] ^ T;
    if (blockIdx.x == 0 && threadIdx.x == 0) d_total[0] = T, d_total[1] = *tot_b;
    // the tile's bursts' workspace entries through LDS, as emit stages them
    __shared__ uint32_t sfirst[kTxsegStage];
    __shared__ uint64_t sboff[kTxsegStage];
    const uint32_t base = blockIdx.x * kTxsegEmitTile;
    const uint32_t last = (seg_cap - base < kTxsegEmitTile ? seg_cap : base + kTxsegEmitTile) - 1;
    const uint32_t lo = (uint32_t)(((uint64_t)base * ratio) >> 32), hi = (uint32_t)(((uint64_t)last * ratio) >> 32);
    const bool staged = hi - lo < kTxsegStage;
    if (staged) {
        for (uint32_t i = threadIdx.x; i <= hi - lo; i += kBlock) sfirst[i] = first[lo + i], sboff[i] = boff[lo + i];
        __syncthreads();
    }
#pragma unroll
    for (uint32_t r = 0; r < kTxsegPerLane; ++r) {
        const uint32_t k = base + r * kBlock + threadIdx.x;
        if (k >= seg_cap) continue;
        const uint32_t i = (uint32_t)(((uint64_t)k * ratio) >> 32);
        if (staged) pattern_record(burst, i, sfirst[i - lo], sboff[i - lo], seg, desc, k);
        else pattern_record(burst, i, first[i], boff[i], seg, desc, k);
    }
}

__global__ __launch_bounds__(kTxsegOneBlock) void pattern_one(const void *__restrict__ burst, uint32_t n,
                                                              uint32_t seg_cap, uint64_t ratio,
                                                              void *__restrict__ seg, void *__restrict__ desc,
                                                              void *__restrict__ res,
                                                              uint64_t *__restrict__ d_total) {
    if (threadIdx.x < n) {
        v4u q1, q2, q3;
        const v4u q0 = burst_words(burst, threadIdx.x, q1, q2, q3);
        const v4u r = {q0.x ^ q1.x, q0.y ^ q1.y, q2.x ^ q3.x, q2.y ^ q3.y};
        *reinterpret_cast<gsv4u *>((uint64_t)res + 16ull * threadIdx.x) = r;
    }
    if (threadIdx.x == 0) d_total[0] = n, d_total[1] = seg_cap;
    for (uint32_t k = threadIdx.x; k < seg_cap; k += kTxsegOneBlock)
        pattern_record(burst, (uint32_t)(((uint64_t)k * ratio) >> 32), k, k, seg, desc, k);
}

}  // namespace

// What a caller without f8 runs on one core: the walk of include/mtcp_gpu_txseg.h
// as a plain loop that writes the 48 B records and the 8 B descriptors of
// packed slots (valid bursts, room for every segment: no status, no room
// test).  Returns the records written.  tools/txseg_bench.py times it and
// holds its output to the model as well.
extern "C" uint64_t txseg_host_loop(const mtcp_gpu_tx_burst *burst, uint32_t n_burst, uint64_t buf_off,
                                    uint32_t off_shift, mtcp_gpu_tx_seg *seg, mtcp_gpu_desc *desc) {
    const uint64_t A = off_shift ? 1ull << off_shift : 2ull;
    uint64_t k = 0, slot = buf_off;
    for (uint32_t i = 0; i < n_burst; ++i) {
        const mtcp_gpu_tx_burst &b = burst[i];
        const uint32_t maxlen = b.mss - 12u;
        uint64_t sent = 0;
        uint16_t ip_id = b.ip_id;
        while (sent < b.len) {
            const uint64_t left = b.len - sent;
            const uint32_t p = left > maxlen ? maxlen : (uint32_t)left;
            if ((uint64_t)b.in_flight + sent + p > b.window) break;
            mtcp_gpu_tx_seg &s = seg[k];
            s.payload_off = b.payload_off + sent;
            s.saddr = b.saddr, s.daddr = b.daddr, s.sport = b.sport, s.dport = b.dport;
            s.seq = b.seq + (uint32_t)sent, s.ack = b.ack, s.ts_val = b.ts_val, s.ts_ecr = b.ts_ecr;
            s.window = b.tcp_window, s.ip_id = ip_id++, s.payload_len = (uint16_t)p, s.mss = b.mss;
            s.flags = MTCP_GPU_TXB_FLAG_ACK, s.form = 1, s.wscale = 0, s.link = b.link;
            desc[k].offset = (uint32_t)(slot >> off_shift), desc[k].len = (uint16_t)(66u + p);
            desc[k].flags = desc[k].rsvd = 0;
            slot += (66u + p + A - 1) & ~(A - 1);
            sent += p;
            ++k;
        }
    }
    return k;
}

// The launches of mtcp_gpu_tx_segment_dev (mtcp_gpu.hip) with the pattern
// kernels: the same form rule, the same grids, d_work laid out the same way.
// n_burst >= 1.  0 on success.
extern "C" int txseg_pattern_launch(const void *d_burst, uint32_t n_burst, void *d_seg, void *d_desc,
                                    uint32_t seg_cap, void *d_res, uint64_t *d_total, void *d_work, void *stream) {
    if (!n_burst || n_burst > seg_cap) return -1;                    // k * ratio stays below 2^64
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 block(mg::kBlock);
    const uint64_t ratio = ((uint64_t)n_burst << 32) / seg_cap;      // k * ratio >> 32 < n_burst for k < seg_cap
    if (n_burst <= mg::kTxsegTile && seg_cap <= mg::kTxsegOneSegs) {
        hipLaunchKernelGGL(pattern_one, dim3(1), dim3(mg::kTxsegOneBlock), 0, st, d_burst, n_burst, seg_cap, ratio, d_seg, d_desc, d_res,
                           d_total);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    auto pad = [](uint64_t v) { return (v + 15) & ~15ull; };
    const uint32_t nwg = (n_burst + mg::kTxsegTile - 1) / mg::kTxsegTile;
    uint8_t *work = static_cast<uint8_t *>(d_work);
    const uint64_t first_off = 16ull * n_burst, boff_off = first_off + pad(4ull * n_burst);
    const uint64_t pc_off = boff_off + pad(8ull * n_burst);
    const uint64_t pb_off = pc_off + pad(4ull * nwg), tot_off = pb_off + pad(8ull * nwg);
    uint32_t *first = reinterpret_cast<uint32_t *>(work + first_off);
    uint64_t *boff = reinterpret_cast<uint64_t *>(work + boff_off);
    uint32_t *part_c = reinterpret_cast<uint32_t *>(work + pc_off);
    uint64_t *part_b = reinterpret_cast<uint64_t *>(work + pb_off);
    unsigned long long *tot_b = reinterpret_cast<unsigned long long *>(work + tot_off);
    uint32_t *tot_c = reinterpret_cast<uint32_t *>(work + tot_off + 8);
    hipLaunchKernelGGL(pattern_plan, dim3(nwg), block, 0, st, d_burst, n_burst, work, part_c, part_b);
    hipLaunchKernelGGL(pattern_scan, dim3(1), block, 0, st, part_c, part_b, nwg, tot_c, tot_b);
    hipLaunchKernelGGL(pattern_place, dim3(nwg), block, 0, st, work, n_burst, part_c, part_b, first, boff, d_res);
    const uint32_t etiles = (seg_cap + mg::kTxsegEmitTile - 1) / mg::kTxsegEmitTile;
    hipLaunchKernelGGL(pattern_emit, dim3(etiles), block, 0, st, d_burst, n_burst, seg_cap, ratio, first, boff, tot_c,
                       tot_b, d_seg, d_desc, d_res, d_total);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
