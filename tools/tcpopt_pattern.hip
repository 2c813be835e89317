// tcpopt_pattern.hip — the memory pattern of the option kernel
// (mtcp_amd/csrc/tcpopt_kernels.hpp) without its walks: the yardstick of
// tools/tcpopt_bench.py.  Measurement infrastructure: nothing here is part
// of libmtcp_gpu.so.
//
// One lane per packet, the option kernel's grid: the same record dwords, the
// same descriptor, and for a TCP_OK frame with doff > 5 the same aligned 16 B
// pieces of the frame (non-temporal), then one 16 B store per packet.  What
// is stored is an XOR of the pieces, so that the loads stay live; no LDS, no
// byte walk, no divergent loop.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const v4u gv4u;

template <bool CMP>
__global__ __launch_bounds__(256) void tcpopt_pattern(const uint8_t *buf, uint64_t buf_len, const uint2 *desc,
                                                      uint32_t n, uint32_t off_shift, const void *res, uint4 *out) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        uint32_t verdict, ihl_doff;
        if constexpr (CMP) {
            const uint32_t w = reinterpret_cast<const uint32_t *>(res)[4 * i + 3];
            ihl_doff = w & 0xFFu, verdict = (w >> 16) & 0xFFu;
        } else {
            const uint2 w = reinterpret_cast<const uint2 *>(res)[5 * i + 4];
            ihl_doff = (w.x >> 16) & 0xFFu, verdict = w.y & 0xFFu;
        }
        const uint2 d = desc[i];
        const uint32_t L = d.y & 0xFFFFu;
        const uint64_t pos = (uint64_t)d.x << off_shift;
        const bool ok = (pos & 1) == 0 && pos + L <= buf_len;
        const int len = 4 * (int)(ihl_doff >> 4) - 20;
        v4u acc = {0, 0, 0, 0};
        if (ok && verdict == 0 && len > 0) {
            const uint32_t first = 34u + 4u * (ihl_doff & 15u);
            const int avail = (int)L - (int)first;
            const uint64_t a = (uint64_t)buf + pos + first;
            const uint32_t o = (uint32_t)a & 15u;
            const int need = min(len + 9, avail);
            const int pieces = need > 0 ? (int)((o + (uint32_t)need + 15u) >> 4) : 0;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < pieces) acc ^= __builtin_nontemporal_load(reinterpret_cast<gv4u *>((a & ~15ull) + 16ull * c));
        }
        out[i] = make_uint4(acc.x, acc.y, acc.z, acc.w);
    }
}

}  // namespace

// Launches the pattern on `stream` with `blocks` workgroups of 256 lanes
// (the caller passes the option kernel's grid).  0, or -1 on a launch error.
extern "C" int tcpopt_pattern_launch(const void *d_buf, uint64_t buf_len, const void *d_desc, uint32_t n,
                                     uint32_t off_shift, const void *d_res, int compact, void *d_out,
                                     uint32_t blocks, void *stream) {
    if (!n) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint8_t *b = static_cast<const uint8_t *>(d_buf);
    const uint2 *d = static_cast<const uint2 *>(d_desc);
    uint4 *o = static_cast<uint4 *>(d_out);
    if (compact)
        hipLaunchKernelGGL(tcpopt_pattern<true>, dim3(blocks), dim3(256), 0, st, b, buf_len, d, n, off_shift, d_res, o);
    else
        hipLaunchKernelGGL(tcpopt_pattern<false>, dim3(blocks), dim3(256), 0, st, b, buf_len, d, n, off_shift, d_res, o);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
