// txbuild_pattern.hip — the yardstick of tools/txbuild_bench.py (measurement
// only, not the product): the frame builder's own memory access pattern
// without its sums, funnel shifts and header shuffles.  Same grid and the same
// group of G lanes per segment as mg::txbuild_kernel (txbuild_kernels.hpp): the
// same record, descriptor and link loads, the same aligned 16 B payload loads
// under the same predicates, the same frame stores (16 B on the destination's
// grid, partial stores in a frame's first and last chunk) and the status byte.
// The bytes stored are the loaded blocks as they are, so the frames it writes
// are not frames; the tool never reads them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../mtcp_amd/csrc/dispatch.hpp"
#include "../mtcp_amd/csrc/txbuild_kernels.hpp"

namespace {

template <int G>
__global__ __launch_bounds__(mg::kBlock) void txbuild_pattern_kernel(const mg::TxBuildParams p) {
    using namespace mg;
    constexpr int kPerWave = kWave / G;
    const int lane = threadIdx.x & (kWave - 1);
    const int t = lane & (G - 1);
    const uint32_t wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const uint32_t nwaves = gridDim.x * kWavesPerBlock;
    for (uint32_t first = wave * kPerWave; first < p.n; first += nwaves * kPerWave) {
        uint32_t i = first + (uint32_t)(lane / G);
        if (G == 64) i = __builtin_amdgcn_readfirstlane(i);
        const bool live = i < p.n;
        if (!live) i = first;
        const uint64_t rec = (uint64_t)p.seg + 48ull * i;
        const v2u r0 = gload64(rec), r1 = gload64(rec + 8), r2 = gload64(rec + 16), r3 = gload64(rec + 24),
                  r4 = gload64(rec + 32), r5 = gload64(rec + 40);
        const v2u d = gload64((uint64_t)p.desc + 8ull * i);
        const uint64_t payload_off = ((uint64_t)r0.y << 32) | r0.x;
        const uint32_t plen = r5.x & 0xFFFFu, flags = r5.y & 0xFFu, link = r5.y >> 24;
        const uint32_t optlen = (flags & 0x02u) ? 20u : 12u;
        const uint32_t L = 54u + optlen + plen;
        const uint64_t off = (uint64_t)d.x << p.off_shift;
        const bool ok = live && !(payload_off > p.payload_bytes || plen > p.payload_bytes - payload_off) &&
                        !((d.y & 0xFFFFu) != L || (off & 1) || off > p.buf_len || L > p.buf_len - off) &&
                        link < p.n_links;
        if (live && t == 0) *reinterpret_cast<gsu8 *>((uint64_t)p.status + i) = (uint8_t)!ok;
        TxSeg s;
        s.status = 0;
        s.dst = (uint64_t)p.buf + off;
        s.src = (uint64_t)p.payload + payload_off;
        s.a = (int)(s.dst & 15);
        s.H = 54 + (int)optlen;
        s.L = (int)L;
        s.plen = plen;
        const int nch = ok ? (s.a + s.L + 15) >> 4 : 0;
        const uint64_t lk = (uint64_t)p.links + 12ull * (link < p.n_links ? link : 0u);
        // the header lanes' words stand in for the header: record and link dwords
        const v4u hdr = {gload32(lk) ^ r1.x, gload32(lk + 4) ^ r2.x ^ r3.x, gload32(lk + 8) ^ r2.y ^ r3.y,
                         r1.y ^ r4.x ^ r4.y};
        const uint64_t end = s.src + s.plen;
        for (int c = t; c < nch; c += G) {
            const int js = 16 * c - s.a;
            const uint64_t from = s.src + (int64_t)(js - s.H);
            const uint64_t blk = from & ~15ull;
            v4u lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
            if ((int64_t)(blk + 16 - s.src) > 0 && (int64_t)(end - blk) > 0) lo = gload_nt(blk);
            if (((uint32_t)from & 15u) && (int64_t)(blk + 32 - s.src) > 0 && (int64_t)(end - blk - 16) > 0)
                hi = gload_nt(blk + 16);
            v4u v = lo | hi;
            if (js < s.H) v |= hdr;
            tx_store(s, c, v);
        }
    }
}

}  // namespace

// The launch of mtcp_gpu_tx_build_dev (mtcp_gpu.hip) with the pattern kernel:
// the same shape rule, the same grid.  0 on success.
extern "C" int txbuild_pattern_launch(const void *d_seg, uint32_t n, const void *d_payload, uint64_t payload_bytes,
                                      const void *d_links, uint32_t n_links, void *d_buf, uint64_t buf_len,
                                      const void *d_desc, uint32_t off_shift, uint8_t *d_status, int num_cu,
                                      void *stream) {
    mg::TxBuildParams p{};
    p.seg = static_cast<const mtcp_gpu_tx_seg *>(d_seg);
    p.payload = static_cast<const uint8_t *>(d_payload);
    p.payload_bytes = payload_bytes;
    p.links = static_cast<const mtcp_gpu_tx_link *>(d_links);
    p.n_links = n_links;
    p.n = n;
    p.buf = static_cast<uint8_t *>(d_buf);
    p.buf_len = buf_len;
    p.desc = static_cast<const mtcp_gpu_desc *>(d_desc);
    p.off_shift = off_shift;
    p.status = d_status;
    if (!n) return 0;
    const int group = txbuild_group(payload_bytes, n);
    const uint32_t per_block = mg::kBlock / group;
    const dim3 grid(std::min<uint32_t>((n + per_block - 1) / per_block, (uint32_t)num_cu * 8));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (group == 64)
        hipLaunchKernelGGL(txbuild_pattern_kernel<64>, grid, dim3(mg::kBlock), 0, st, p);
    else if (group == 32)
        hipLaunchKernelGGL(txbuild_pattern_kernel<32>, grid, dim3(mg::kBlock), 0, st, p);
    else if (group == 16)
        hipLaunchKernelGGL(txbuild_pattern_kernel<16>, grid, dim3(mg::kBlock), 0, st, p);
    else
        hipLaunchKernelGGL(txbuild_pattern_kernel<8>, grid, dim3(mg::kBlock), 0, st, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
