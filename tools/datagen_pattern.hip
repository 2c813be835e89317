// datagen_pattern.hip — the memory pattern of the data generation's two kernels
// (mtcp_amd/csrc/datagen_kernels.hpp) without their arithmetic: the yardstick
// of tools/datagen_bench.py.  Measurement infrastructure: nothing here is part
// of libmtcp_gpu.so.
//
// pattern_burst takes the segments as the burst kernel does (the lanes' own
// loops, then the wave over the long lists, 64 flag dwords a step), loads the
// same d_dtx record, tx record, state pieces and send-state pieces, indices and
// flag dwords, and stores the same 64 B burst and parked dword; what it stores
// are the loaded words themselves: no fold, no BAD test, no status chain.  The
// burst's fields are copies (seq = snd_nxt, len = the sb_len field, in_flight =
// the snd_una field, window = the cwnd field, payload_off = sb_off), so row f8
// behind it has the call's own fan-out only where the caller passes records
// that already hold those values (the bench tool makes them from the call's own
// bursts).  Row f8's launches have no pattern here: the tool runs the library's
// mtcp_gpu_tx_segment_dev between the two.  pattern_commit loads the parked
// dword, row f8's 16 B result and the same six dwords of the stream's records
// and stores them back where the commit kernel stores, with the 16 B result,
// without the commit's arithmetic; every field the pattern reads keeps its value.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mtcp_amd/csrc/datagen_kernels.hpp"

namespace {

using namespace mg;

__global__ __launch_bounds__(kBlock) void pattern_burst(
    const uint8_t *__restrict__ ack, const uint32_t *__restrict__ idx, const DataGenParams P,
    const uint32_t *__restrict__ seg_sid, const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ nseg,
    const uint32_t *__restrict__ seg_stop, const uint32_t *__restrict__ ack_stop, const uint8_t *__restrict__ state,
    const uint8_t *__restrict__ snd, const uint8_t *__restrict__ tx, const uint8_t *__restrict__ dtx,
    uint8_t *__restrict__ burst, uint32_t *__restrict__ park) {
    const uint32_t n = P.n, m = min(nseg[0], n);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const bool valid = j < m;
    uint32_t start = 0, end = 0, sid = 0xFFFFFFFFu;
    if (valid) {
        start = min(seg_start[j], n);
        end = max(min(seg_start[j + 1], n), start);
        sid = seg_sid[j];
    }
    const bool is_stream = valid && sid <= P.max_id;
    v4u d = {0, 0, 0, 0}, a = d, b = d, r0 = d, r1 = d, q0 = d, q1 = d, q4 = {0, 0, 0, 13};
    v2u q5 = {0, 0};
    uint32_t stopc = start;
    if (is_stream) {
        d = gload((uint64_t)dtx + 16ull * sid);
        a = gload((uint64_t)tx + 32ull * sid), b = gload((uint64_t)tx + 32ull * sid + 16);
        r0 = gload((uint64_t)state + 64ull * sid), r1 = gload((uint64_t)state + 64ull * sid + 16);
        const uint64_t sa = (uint64_t)snd + 128ull * sid;
        q0 = gload(sa), q1 = gload(sa + 16), q4 = gload(sa + 64), q5 = gload64(sa + 80);
        stopc = min(max(ack_stop[j] + (seg_stop[j] & 0u), start), end);
    }
    uint32_t f = 0;
    const bool lng = stopc - start > kDatagenLaneMax;
    if (!lng) {
        for (uint32_t p = start; p < stopc; ++p) {
            const uint32_t q = idx[p];
            if (q >= n) continue;
            f += gload32((uint64_t)ack + 16ull * q + 12);
        }
    }
    uint64_t todo = __ballot(lng);
    while (todo) {
        const int l = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t lstart = rcv_bcast(start, l), lend = rcv_bcast(stopc, l);
        uint32_t lf = 0;
        for (uint32_t base = lstart; base < lend; base += kWave) {
            uint32_t w = 0;
            if (lane < lend - base) {
                const uint32_t q = idx[base + lane];
                if (q < n) w = gload32((uint64_t)ack + 16ull * q + 12);
            }
            lf += (uint32_t)__popcll(__ballot(w >> 31));           // one value out of the step's 64 loads
        }
        if ((int)lane == l) f = lf;
    }
    if (j < n) {
        const uint64_t at = (uint64_t)burst + 64ull * j;
        const v4u b0 = {d.x, d.y, a.x, a.y}, b1 = {a.z, q0.x, r0.x, P.cur_ts};
        const v4u b2 = {r1.y, q4.y, q0.y, q1.w}, b3 = {q0.w, a.w << 16, q4.w & 0xFFFFu, b.z};
        *reinterpret_cast<gsv4u *>(at) = b0;
        *reinterpret_cast<gsv4u *>(at + 16) = b1;
        *reinterpret_cast<gsv4u *>(at + 32) = b2;
        *reinterpret_cast<gsv4u *>(at + 48) = b3;
    }
    if (valid) park[j] = f + d.z + d.w + b.x + b.y + r0.y + r1.w + q4.x + q4.z + q5.x + q5.y;
}

__global__ __launch_bounds__(kBlock) void pattern_commit(
    const uint32_t *__restrict__ park, const uint8_t *__restrict__ f8res, const DataGenParams P,
    const uint32_t *__restrict__ seg_sid, const uint32_t *__restrict__ nseg, uint8_t *__restrict__ snd,
    uint8_t *__restrict__ tx, uint8_t *__restrict__ dtx, mtcp_gpu_datagen_res *__restrict__ dres) {
    const uint32_t m = min(nseg[0], P.n);
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= m) return;
    const uint32_t sid = seg_sid[k];
    const uint32_t pk = park[k];
    v4u r = gload((uint64_t)f8res + 16ull * k);
    if (sid <= P.max_id) {
        const uint64_t sa = (uint64_t)snd + 128ull * sid, ta = (uint64_t)tx + 32ull * sid;
        const uint32_t snd_nxt = gload32(sa), rto = gload32(sa + 36), bits2 = gload32(sa + 84);
        const uint32_t id_cnt = gload32(ta + 12), misc = gload32(ta + 16), ts_last = gload32(ta + 20);
        uint32_t *srec = reinterpret_cast<uint32_t *>(snd + 128ull * sid);
        uint32_t *trec = reinterpret_cast<uint32_t *>(tx + 32ull * sid);
        srec[0] = snd_nxt, srec[10] = rto, snd[128ull * sid + 85] = (uint8_t)(bits2 >> 8);
        trec[3] = id_cnt, trec[4] = misc, trec[5] = ts_last;
        dtx[16ull * sid + 12] = (uint8_t)(pk & 1u);
        r.w += pk;
    }
    *reinterpret_cast<gsv4u *>((uint64_t)dres + 16ull * k) = r;
}

}  // namespace

// The burst kernel's pattern for a grouped batch, on `stream`: the arguments
// of mtcp_gpu_datagen_dev's first launch; d_work as
// mtcp_gpu_datagen_work_bytes sizes it (the bursts at its start, row f8's
// results and the parked dwords behind them).  0, or -1 on a launch error.
extern "C" int datagen_pattern_burst(const void *d_ack, const void *d_ack_stop, uint32_t n, uint32_t max_id,
                                     const void *d_idx, const void *d_seg_sid, const void *d_seg_start,
                                     const void *d_nseg, const void *d_seg_stop, const void *d_state, const void *d_snd,
                                     const void *d_tx, const void *d_dtx, void *d_work, void *stream) {
    if (!n) return 0;
    const DataGenWork w = datagen_work(n);
    uint8_t *work = static_cast<uint8_t *>(d_work);
    const DataGenParams P{n, max_id, 256, 0x12345678u};
    const auto u8 = [](const void *p) { return static_cast<const uint8_t *>(p); };
    const auto u32 = [](const void *p) { return static_cast<const uint32_t *>(p); };
    hipLaunchKernelGGL(pattern_burst, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       u8(d_ack), u32(d_idx), P, u32(d_seg_sid), u32(d_seg_start), u32(d_nseg), u32(d_seg_stop),
                       u32(d_ack_stop), u8(d_state), u8(d_snd), u8(d_tx), u8(d_dtx), work + w.burst_off,
                       reinterpret_cast<uint32_t *>(work + w.park_off));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The commit kernel's pattern, same workspace.  0, or -1 on a launch error.
extern "C" int datagen_pattern_commit(uint32_t n, uint32_t max_id, const void *d_seg_sid, const void *d_nseg, void *d_snd,
                                      void *d_tx, void *d_dtx, void *d_dres, void *d_work, void *stream) {
    if (!n) return 0;
    const DataGenWork w = datagen_work(n);
    uint8_t *work = static_cast<uint8_t *>(d_work);
    const DataGenParams P{n, max_id, 256, 0x12345678u};
    hipLaunchKernelGGL(pattern_commit, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint32_t *>(work + w.park_off), work + w.res_off, P,
                       static_cast<const uint32_t *>(d_seg_sid), static_cast<const uint32_t *>(d_nseg),
                       static_cast<uint8_t *>(d_snd), static_cast<uint8_t *>(d_tx), static_cast<uint8_t *>(d_dtx),
                       static_cast<mtcp_gpu_datagen_res *>(d_dres));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Byte offsets of the workspace's parts for n indices: the bursts, row f8's
// results, the parked dwords, row f8's own workspace.
extern "C" void datagen_pattern_offsets(uint32_t n, uint64_t out[4]) {
    const DataGenWork w = datagen_work(n);
    out[0] = w.burst_off, out[1] = w.res_off, out[2] = w.park_off, out[3] = w.f8_off;
}
