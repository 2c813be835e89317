// ackwalk_pattern.hip — the memory pattern of the ProcessACK walk
// (mtcp_amd/csrc/ackwalk_kernels.hpp) without the walk, and the same walk as a
// plain loop on one host core: the yardsticks of tools/ackwalk_bench.py.
// Measurement infrastructure: nothing here is part of libmtcp_gpu.so.
//
// The pattern: the same two launches on the same grids.  The gather has no
// arithmetic to leave out and is the library's kernel.  pattern_walk takes the
// segments as the walker does (the lanes' rounds, then the wave over what is
// left of the last few, 64 inputs a step), loads the same state, inputs and
// indices and stores the same ACK records, state pieces and stop positions;
// what it stores is a sum of what it loaded: no comparison, no division, and
// in the wave form no step-by-step broadcast.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../mtcp_amd/csrc/ackwalk_kernels.hpp"

namespace {

using namespace mg;

template <uint32_t SHORT, uint32_t WAVE_MAX>
__global__ __launch_bounds__(kBlock) void pattern_walk(const uint4 *__restrict__ win, const uint32_t *__restrict__ idx,
                                                       uint32_t n, uint32_t max_id,
                                                       const uint32_t *__restrict__ seg_sid,
                                                       const uint32_t *__restrict__ seg_start,
                                                       const uint32_t *__restrict__ nseg, uint4 *__restrict__ snd,
                                                       uint4 *__restrict__ ack, uint32_t *__restrict__ ack_stop) {
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
    AckState s{};
    if (is_stream) ack_load_state(s, snd + 8ull * sid);
    uint32_t mid = start;
    uint64_t todo;
    do {
        const uint32_t lim = end - mid > SHORT ? mid + SHORT : end;
        for (; mid < lim; ++mid) {
            const uint32_t p = idx[mid];
            if (p >= n) continue;
            const uint4 v = win[mid];
            s.snd_nxt += v.x, s.cwnd += v.w;
            ack[p] = make_uint4(v.y, s.snd_nxt, s.cwnd, v.z);
        }
        todo = __ballot(mid < end);
    } while ((uint32_t)__popcll(todo) > WAVE_MAX);
    while (todo) {
        const int l = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t lstart = rcv_bcast(mid, l), lend = rcv_bcast(end, l);
        uint32_t acc = rcv_bcast(s.snd_nxt, l);
        for (uint32_t base = lstart; base < lend; base += kWave) {
            if (base + lane < lend) {
                const uint4 v = win[base + lane];
                const uint32_t p = idx[base + lane];
                acc += v.x;
                if (p < n) ack[p] = make_uint4(v.y, acc, v.w, v.z);
            }
        }
        if ((int)lane == l) s.snd_nxt = acc;
    }
    if (is_stream) ack_store_state(s, snd + 8ull * sid, 3u);
    if (valid) ack_stop[j] = end;
}

}  // namespace

// The walk's pattern for a grouped batch, on `stream`; the arguments of
// mtcp_gpu_ackwalk_dev less cur_ts.  0, or -1 on a launch error.
extern "C" int ackwalk_pattern_launch(const void *d_res, const void *d_opt, const void *d_place, uint32_t n,
                                      uint32_t max_id, const void *d_idx, const void *d_seg_sid,
                                      const void *d_seg_start, const void *d_nseg, void *d_snd, void *d_ack,
                                      void *d_ack_stop, void *d_work, void *stream) {
    if (!n) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 block(kBlock), grid((n + kBlock - 1) / kBlock);
    uint4 *win = static_cast<uint4 *>(d_work);
    hipLaunchKernelGGL(ackwalk_gather_kernel, grid, block, 0, st, static_cast<const uint8_t *>(d_res),
                       static_cast<const uint4 *>(d_opt), static_cast<const uint4 *>(d_place),
                       static_cast<const uint32_t *>(d_idx), n, win, static_cast<uint4 *>(d_ack));
    hipLaunchKernelGGL((pattern_walk<kAckShortLen, kAckWaveMax>), grid, block, 0, st, win,
                       static_cast<const uint32_t *>(d_idx), n, max_id, static_cast<const uint32_t *>(d_seg_sid),
                       static_cast<const uint32_t *>(d_seg_start), static_cast<const uint32_t *>(d_nseg),
                       static_cast<uint4 *>(d_snd), static_cast<uint4 *>(d_ack), static_cast<uint32_t *>(d_ack_stop));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The same walk as a plain loop on the calling core, over host memory: the
// arguments of mtcp_gpu_ackwalk with m = nseg[0].  ack_step is the kernels' own
// step function compiled for the host, so tests/test_ackwalk_model.py can hold
// it against the model where there is no GPU.
extern "C" void ackwalk_host_loop(const mtcp_gpu_result *res, const mtcp_gpu_tcpopt *opt,
                                  const mtcp_gpu_rcv_place *place, uint32_t n, uint32_t max_id, const uint32_t *idx,
                                  const uint32_t *seg_sid, const uint32_t *seg_start, uint32_t m, uint32_t cur_ts,
                                  mtcp_gpu_ack_state *snd, mtcp_gpu_ack_rec *ack, uint32_t *ack_stop) {
    memset(ack, 0, (size_t)n * sizeof(*ack));
    for (uint32_t j = 0; j < m && j < n; ++j) {
        const uint32_t start = seg_start[j] < n ? seg_start[j] : n;
        const uint32_t end = seg_start[j + 1] < n ? (seg_start[j + 1] > start ? seg_start[j + 1] : start) : n;
        const uint32_t sid = seg_sid[j];
        if (sid > max_id) {
            ack_stop[j] = start;
            continue;
        }
        AckState s;
        memcpy(&s, snd + sid, sizeof(s));
        bool deferred = false;
        uint32_t dirty = 0, stop = end;
        for (uint32_t k = start; k < end; ++k) {
            const uint32_t p = idx[k];
            if (p >= n) continue;
            const uint32_t pv = place[p].verdict;
            uint32_t bits = res[p].payload_len == 0 ? kAckInNoPayload : 0u;
            if (pv >= MTCP_GPU_RCV_ACK_ONLY && pv <= MTCP_GPU_RCV_PUT_STORED) bits |= kAckInValid;
            else if (!(pv >= MTCP_GPU_RCV_PAWS_NO_TS && pv <= MTCP_GPU_RCV_SEQ_AHEAD)) bits |= kAckInRcvDeferred;
            if (opt && (opt[p].flags & MTCP_GPU_TCPOPT_TS_FOUND)) bits |= kAckInHasTs;
            uint4 in;
            in.x = res[p].seq, in.y = res[p].ack_seq, in.z = opt ? opt[p].ts_ref : 0;
            in.w = res[p].window | (uint32_t)res[p].tcp_flags << 16 | bits << 24;
            const uint4 rec = ack_step(s, in, cur_ts, deferred);
            if (deferred) stop = k < stop ? k : stop;
            else dirty |= ack_dirty(rec);
            memcpy(ack + p, &rec, sizeof(rec));
        }
        if (dirty) memcpy(snd + sid, &s, sizeof(s));
        ack_stop[j] = stop;
    }
}
