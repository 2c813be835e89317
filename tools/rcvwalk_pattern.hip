// rcvwalk_pattern.hip — the memory pattern of the receive walk
// (mtcp_amd/csrc/rcvwalk_kernels.hpp) without the walk, the same walk as a
// plain loop on one host core, and the walk kernel at other round lengths and
// take-over counts: the yardsticks of tools/rcvwalk_bench.py.  Measurement
// infrastructure: nothing here is part of libmtcp_gpu.so.
//
// The pattern: the same two launches on the same grids.  The gather has no
// arithmetic to leave out and is the library's kernel.  pattern_walk takes the
// segments as the walker does (the lanes' rounds, then the wave over what is left
// of the last few, 64 inputs a step), loads the same state, inputs and indices and
// stores the same placement records, state records and stop positions; what it
// stores is a sum of what it loaded: no comparison, no fragment work, and in
// the wave form no step-by-step broadcast.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../mtcp_amd/csrc/rcvwalk_kernels.hpp"

namespace {

using namespace mg;

template <uint32_t SHORT, uint32_t WAVE_MAX>
__global__ __launch_bounds__(kBlock) void pattern_walk(const uint4 *__restrict__ win, const uint32_t *__restrict__ idx,
                                                       uint32_t n, uint32_t max_id,
                                                       const uint32_t *__restrict__ seg_sid,
                                                       const uint32_t *__restrict__ seg_start,
                                                       const uint32_t *__restrict__ nseg, uint4 *__restrict__ state,
                                                       uint4 *__restrict__ place, uint32_t *__restrict__ seg_stop) {
    const uint32_t m = min(nseg[0], n);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t j0 = (blockIdx.x * kBlock + threadIdx.x) - lane;
    if (j0 >= m) return;
    const uint32_t j = j0 + lane;
    const bool valid = j < m;
    uint32_t start = 0, end = 0, sid = 0xFFFFFFFFu;
    if (valid) {
        start = min(seg_start[j], n);
        end = max(min(seg_start[j + 1], n), start);
        sid = seg_sid[j];
    }
    const bool is_stream = valid && sid <= max_id;
    if (!is_stream) end = start;
    RcvState s{};
    if (is_stream) rcv_load_state(s, state + 4ull * sid);
    uint32_t mid = start;
    uint64_t todo;
    do {
        const uint32_t lim = end - mid > SHORT ? mid + SHORT : end;
        for (; mid < lim; ++mid) {
            const uint32_t p = idx[mid];
            if (p >= n) continue;
            const uint4 v = win[mid];
            s.rcv_nxt += v.x, s.rcv_wnd += v.w;
            place[p] = make_uint4(v.y, s.rcv_nxt, s.rcv_wnd, v.z);
        }
        todo = __ballot(mid < end);
    } while ((uint32_t)__popcll(todo) > WAVE_MAX);
    while (todo) {
        const int l = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t lstart = rcv_bcast(mid, l), lend = rcv_bcast(end, l);
        uint32_t acc = rcv_bcast(s.rcv_nxt, l);
        for (uint32_t base = lstart; base < lend; base += kWave) {
            if (base + lane < lend) {
                const uint4 v = win[base + lane];
                const uint32_t p = idx[base + lane];
                acc += v.x;
                if (p < n) place[p] = make_uint4(v.y, acc, v.w, v.z);
            }
        }
        if ((int)lane == l) s.rcv_nxt = acc;
    }
    if (is_stream) rcv_store_state(s, state + 4ull * sid);
    if (valid) seg_stop[j] = end;
}

template <uint32_t SHORT, uint32_t WAVE_MAX>
int launch_walk(hipStream_t st, const uint4 *win, const uint32_t *idx, uint32_t n, uint32_t max_id,
                const uint32_t *seg_sid, const uint32_t *seg_start, const uint32_t *nseg, uint32_t has_opt,
                uint4 *state, uint4 *place, uint32_t *seg_stop) {
    hipLaunchKernelGGL((rcvwalk_walk_kernel<SHORT, WAVE_MAX>), dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, win, idx, n,
                       max_id, seg_sid, seg_start, nseg, has_opt, state, place, seg_stop);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace

// The walk's pattern for a grouped batch, on `stream`; the arguments of
// mtcp_gpu_rcvwalk_dev.  0, or -1 on a launch error.
extern "C" int rcvwalk_pattern_launch(const void *d_res, const void *d_opt, uint32_t n, uint32_t max_id,
                                      const void *d_idx, const void *d_seg_sid, const void *d_seg_start,
                                      const void *d_nseg, void *d_state, void *d_place, void *d_seg_stop, void *d_work,
                                      void *stream) {
    if (!n) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 block(kBlock), grid((n + kBlock - 1) / kBlock);
    uint4 *win = static_cast<uint4 *>(d_work);
    hipLaunchKernelGGL(rcvwalk_gather_kernel, grid, block, 0, st, static_cast<const uint8_t *>(d_res),
                       static_cast<const uint4 *>(d_opt), static_cast<const uint32_t *>(d_idx), n, win,
                       static_cast<uint4 *>(d_place));
    hipLaunchKernelGGL((pattern_walk<kRcvShortLen, kRcvWaveMax>), grid, block, 0, st, win, static_cast<const uint32_t *>(d_idx), n,
                       max_id, static_cast<const uint32_t *>(d_seg_sid), static_cast<const uint32_t *>(d_seg_start),
                       static_cast<const uint32_t *>(d_nseg), static_cast<uint4 *>(d_state),
                       static_cast<uint4 *>(d_place), static_cast<uint32_t *>(d_seg_stop));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The library's two launches with the walker's round length and take-over
// count set to one of the pairs below (0xFFFFFFFF: every segment by its lane
// alone).  0, -1 on a launch error, -2 for another pair.
extern "C" int rcvwalk_variant_launch(uint32_t short_len, uint32_t wave_max, const void *d_res, const void *d_opt,
                                      uint32_t n, uint32_t max_id, const void *d_idx, const void *d_seg_sid,
                                      const void *d_seg_start, const void *d_nseg, void *d_state, void *d_place,
                                      void *d_seg_stop, void *d_work, void *stream) {
    if (!n) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    uint4 *win = static_cast<uint4 *>(d_work);
    const uint32_t *idx = static_cast<const uint32_t *>(d_idx), *ssid = static_cast<const uint32_t *>(d_seg_sid);
    const uint32_t *sstart = static_cast<const uint32_t *>(d_seg_start), *nseg = static_cast<const uint32_t *>(d_nseg);
    uint4 *state = static_cast<uint4 *>(d_state), *place = static_cast<uint4 *>(d_place);
    uint32_t *stop = static_cast<uint32_t *>(d_seg_stop);
    const uint32_t has_opt = d_opt ? 1u : 0u;
    hipLaunchKernelGGL(rcvwalk_gather_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st,
                       static_cast<const uint8_t *>(d_res), static_cast<const uint4 *>(d_opt), idx, n, win, place);
#define VARIANT(S, W)                        \
    if (short_len == S && wave_max == W)     \
    return launch_walk<S, W>(st, win, idx, n, max_id, ssid, sstart, nseg, has_opt, state, place, stop)
    VARIANT(32u, 0u);
    VARIANT(32u, 1u);
    VARIANT(32u, 3u);
    VARIANT(32u, 8u);
    VARIANT(8u, 3u);
    VARIANT(128u, 3u);
    VARIANT(0xFFFFFFFFu, 0u);
#undef VARIANT
    return -2;
}

// The same walk as a plain loop on the calling core, over host memory: the
// arguments of mtcp_gpu_rcvwalk with m = nseg[0].  rcv_step is the kernels' own
// step function compiled for the host, so tests/test_rcvwalk_model.py can hold
// it against the model where there is no GPU.
extern "C" void rcvwalk_host_loop(const mtcp_gpu_result *res, const mtcp_gpu_tcpopt *opt, uint32_t n,
                                  uint32_t max_id, const uint32_t *idx, const uint32_t *seg_sid,
                                  const uint32_t *seg_start, uint32_t m, mtcp_gpu_rcv_state *state,
                                  mtcp_gpu_rcv_place *place, uint32_t *seg_stop) {
    memset(place, 0, (size_t)n * sizeof(*place));
    for (uint32_t j = 0; j < m && j < n; ++j) {
        const uint32_t start = seg_start[j] < n ? seg_start[j] : n;
        const uint32_t end = seg_start[j + 1] < n ? (seg_start[j + 1] > start ? seg_start[j + 1] : start) : n;
        const uint32_t sid = seg_sid[j];
        if (sid > max_id) {
            seg_stop[j] = start;
            continue;
        }
        RcvState s;
        const uint32_t *r = reinterpret_cast<const uint32_t *>(state + sid);
        s.rcv_nxt = r[0], s.rcv_wnd = r[1], s.head_seq = r[2], s.merged_len = r[3];
        s.size = r[4], s.ts_recent = r[5], s.ts_lastack = r[6], s.bits = r[7];
        for (int k = 0; k < MTCP_GPU_RCV_MAX_FRAGS; ++k) s.fs[k] = r[8 + 2 * k], s.fl[k] = r[9 + 2 * k];
        bool deferred = false, dirty = false;
        uint32_t stop = end;
        for (uint32_t k = start; k < end; ++k) {
            const uint32_t p = idx[k];
            if (p >= n) continue;
            uint4 in;
            in.x = res[p].seq, in.y = opt ? opt[p].ts_val : 0, in.z = opt ? opt[p].ts_ref : 0;
            in.w = res[p].payload_len | (uint32_t)res[p].tcp_flags << 16 | (opt ? (uint32_t)opt[p].flags << 24 : 0);
            const uint4 rec = rcv_step(s, in, opt != nullptr, deferred);
            if (deferred) stop = k < stop ? k : stop;
            else dirty = true;
            memcpy(place + p, &rec, sizeof(rec));
        }
        if (dirty) {
            uint32_t *w = reinterpret_cast<uint32_t *>(state + sid);
            w[0] = s.rcv_nxt, w[1] = s.rcv_wnd, w[2] = s.head_seq, w[3] = s.merged_len;
            w[4] = s.size, w[5] = s.ts_recent, w[6] = s.ts_lastack, w[7] = s.bits;
            for (int k = 0; k < MTCP_GPU_RCV_MAX_FRAGS; ++k) w[8 + 2 * k] = s.fs[k], w[9 + 2 * k] = s.fl[k];
        }
        seg_stop[j] = stop;
    }
}
