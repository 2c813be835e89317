// rcvcopy_pattern.hip — the memory pattern of the receive copy
// (mtcp_amd/csrc/rcvcopy_kernels.hpp) without plan, shift or ordering, the
// plan's step functions as a plain loop on the host, and one host core doing
// the same copies with memcpy: the yardsticks of tools/rcvcopy_bench.py and of
// tests/test_rcvcopy_model.py.  Measurement infrastructure: nothing here is
// part of libmtcp_gpu.so.
//
// The pattern: G lanes per position on the front kernel's grid.  A position
// with a length loads the aligned 16 B pieces its source run touches, each
// chunk its two, non-temporal, and stores one aligned 16 B piece per chunk of
// the destination's grid; what it stores is the sum of the two pieces.  No
// class, no segment lookup, no shift, no partial store: the chunks at a run's
// ends are stored whole, so it runs on an arena of its own.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../mtcp_amd/csrc/dispatch.hpp"
#include "../mtcp_amd/csrc/rcvcopy_kernels.hpp"

namespace {

using namespace mg;

// run[pos]: source byte offset lo, hi; destination byte offset >> 4 (the first chunk); chunks | 0
template <int G>
__global__ __launch_bounds__(kBlock) void pattern_front(uint64_t buf, uint64_t buf_len, const uint4 *__restrict__ run,
                                                        uint32_t n, uint64_t arena, uint64_t arena_bytes) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t pos = t / G, sub = t % G;
    if (pos >= n) return;
    const uint4 r = run[pos];
    const uint64_t s0 = ((uint64_t)r.y << 32 | r.x) & ~15ull, d0 = (uint64_t)r.z << 4;
    for (uint32_t c = sub; c < r.w; c += G) {
        const uint64_t s = s0 + 16ull * c, d = d0 + 16ull * c;
        v4u v = {0u, 0u, 0u, 0u};
        if (s + 16 <= buf_len) v = gload_nt(buf + s);
        if (s + 32 <= buf_len) {
            const v4u h = gload_nt(buf + s + 16);
            v.x += h.x, v.y += h.y, v.z += h.z, v.w += h.w;
        }
        if (d + 16 <= arena_bytes) *reinterpret_cast<gsv4u *>(arena + d) = v;
    }
}

}  // namespace

extern "C" {

int rcvcopy_pattern_dev(const void *d_buf, uint64_t buf_len, const void *d_run, uint32_t n, void *d_arena,
                        uint64_t arena_bytes, int group, void *stream) {
    if (!n) return 0;
    const dim3 block(kBlock), grid((uint32_t)(((uint64_t)n * group + kBlock - 1) / kBlock));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t buf = reinterpret_cast<uint64_t>(d_buf), arena = reinterpret_cast<uint64_t>(d_arena);
    if (group == 8)
        hipLaunchKernelGGL(pattern_front<8>, grid, block, 0, st, buf, buf_len, static_cast<const uint4 *>(d_run), n, arena, arena_bytes);
    else if (group == 32)
        hipLaunchKernelGGL(pattern_front<32>, grid, block, 0, st, buf, buf_len, static_cast<const uint4 *>(d_run), n, arena, arena_bytes);
    else
        return -22;
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

// The library's width rule (dispatch.hpp rcvcopy_group).
int rcvcopy_group_of(uint64_t buf_len, uint32_t n) { return rcvcopy_group(buf_len, n); }

// prep and plan on the host, with the kernels' own step functions: cstat[n]
// and rbuf[max_id + 1] as mtcp_gpu_rcvcopy_dev leaves them; moved[m]: the
// segment's stream compacts.  No byte is copied.
void rcvcopy_host_plan(const uint8_t *res, const uint32_t *place, const uint32_t *desc, uint32_t off_shift,
                       uint64_t buf_len, uint32_t n, uint32_t max_id, const uint32_t *idx, const uint32_t *seg_sid,
                       const uint32_t *seg_start, uint32_t m, const uint32_t *seg_stop, uint32_t *rbuf,
                       uint64_t arena_bytes, uint8_t *cstat, uint8_t *moved) {
    memset(cstat, 0, n);
    for (uint32_t j = 0; j < m && j < n; ++j) {
        moved[j] = 0;
        const uint32_t sid = seg_sid[j];
        if (sid > max_id) continue;
        const uint32_t start = seg_start[j] < n ? seg_start[j] : n;
        uint32_t end = seg_start[j + 1] < n ? seg_start[j + 1] : n;
        if (end < start) end = start;
        uint32_t stop = seg_stop[j] > start ? seg_stop[j] : start;
        if (stop > end) stop = end;
        uint32_t *r = rbuf + 8ull * sid;
        CopyBuf b{(uint64_t)r[1] << 32 | r[0], r[2], r[3], r[4], r[5], r[6], r[7]};
        const bool bad = copy_buf_bad(b, arena_bytes);
        CopyPlan pl{0u, 0u, false};
        for (uint32_t pos = start; pos < stop; ++pos) {
            const uint32_t p = idx[pos];
            if (p >= n) continue;
            uint64_t src;
            const uint32_t w8 = reinterpret_cast<const uint32_t *>(res + 40ull * p)[8];
            const uint32_t code = copy_src(place[4ull * p + 3], w8, desc[2ull * p], desc[2ull * p + 1] & 0xFFFFu,
                                           off_shift, buf_len, src);
            if (code == 0) continue;
            cstat[p] = (uint8_t)copy_step(pl, bad, b.size, place[4ull * p], place[4ull * p + 3] & 0xFFFFu, code);
        }
        moved[j] = copy_finish(pl, b);
        if (pl.any) r[3] = b.head, r[4] = b.tail, r[5] = b.last;
    }
}

// One host core: the same copies with memcpy from the staged frames.
void rcvcopy_host_memcpy(const uint8_t *buf, const uint64_t *src, const uint64_t *dst, const uint32_t *len,
                         uint32_t n, uint8_t *arena) {
    for (uint32_t i = 0; i < n; ++i)
        if (len[i]) memcpy(arena + dst[i], buf + src[i], len[i]);
}

}  // extern "C"
