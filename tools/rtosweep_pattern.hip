// rtosweep_pattern.hip — the memory pattern of the retransmission-timeout sweep's
// kernels (mtcp_amd/csrc/rtosweep_kernels.hpp) without their arithmetic, and the
// sweep's three launches with the due test in its other form (ts_rto loaded only
// where on_rto is 1): the yardsticks of tools/rtosweep_bench.py.  Measurement infrastructure: nothing here is part
// of libmtcp_gpu.so.
//
// pattern_count takes the streams as the count kernel does (a lane per stream,
// 16 rounds, a wave owns 1 024 consecutive ids), loads dword 21 and dword 10 of
// every record as the count kernel does, and stores
// 128 B and one dword per wave; what it stores are sums of the loaded words: no
// test against cur_ts, no ballot, no popcount.  pattern_emit loads the wave's 128 B and its
// dword as the emit kernel does and, for a stream whose bit is set in the masks
// the caller left there (the sweep's own: the tool runs the sweep first and
// keeps its workspace), loads bytes 0-87 of the record and the 16 B d_dtx record
// and stores the six dwords and the byte the step may store, the 16 B result and
// the d_seg_sid entry: the loaded words themselves, at entry id >> shift
// instead of a rank (the tool's due streams are the multiples of 1 << shift, so
// that is the sweep's own entry), without rto_step.  Both zero the table as the
// sweep does.  The scan between them is the sweep's own launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mtcp_amd/csrc/rtosweep_kernels.hpp"

namespace {

using namespace mg;

__global__ __launch_bounds__(kBlock) void pattern_count(const uint8_t *__restrict__ snd, const RtoSweepParams P,
                                                        uint64_t *__restrict__ sums, uint32_t *__restrict__ cnt) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const uint64_t base = (uint64_t)wave * kRtoWaveChunk + lane;
    uint64_t s = 0;
#pragma unroll
    for (int r = 0; r < kRtoRounds; ++r) {
        const uint64_t id = base + (uint32_t)r * kWave;
        if (id <= P.max_id)
            s += (uint64_t)gload32((uint64_t)snd + 128ull * id + 84) << 32 | gload32((uint64_t)snd + 128ull * id + 40);
    }
    if (lane < (uint32_t)kRtoRounds) sums[(uint64_t)wave * kRtoRounds + lane] = s;
    if (lane == 0) cnt[wave] = (uint32_t)s;
}

// rto_count_kernel with the due test's other form: dword 10 only where dword 21
// says on_rto == 1, behind that load.
__global__ __launch_bounds__(kBlock) void cond_count_kernel(const uint8_t *__restrict__ snd, const RtoSweepParams P,
                                                            uint64_t *__restrict__ ballots, uint32_t *__restrict__ cnt) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const uint64_t base = (uint64_t)wave * kRtoWaveChunk + lane;
    uint32_t b2[kRtoRounds], ts[kRtoRounds];
#pragma unroll
    for (int r = 0; r < kRtoRounds; ++r) {
        const uint64_t id = base + (uint32_t)r * kWave;
        b2[r] = 0, ts[r] = 0;
        if (id <= P.max_id) b2[r] = gload32((uint64_t)snd + 128ull * id + 84);
    }
#pragma unroll
    for (int r = 0; r < kRtoRounds; ++r)
        if (rto_on(b2[r])) ts[r] = gload32((uint64_t)snd + 128ull * (base + (uint32_t)r * kWave) + 40);
    uint64_t mine = 0;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kRtoRounds; ++r) {
        const uint64_t m = __ballot(rto_due(b2[r], ts[r], P.cur_ts));
        c += (uint32_t)__popcll(m);
        if ((int)lane == r) mine = m;
    }
    if (lane < (uint32_t)kRtoRounds) ballots[(uint64_t)wave * kRtoRounds + lane] = mine;
    if (lane == 0) cnt[wave] = c;
}

__global__ __launch_bounds__(kBlock) void pattern_emit(const uint64_t *__restrict__ ballots,
                                                       const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ tot,
                                                       const RtoSweepParams P, uint32_t shift, uint8_t *__restrict__ snd,
                                                       uint8_t *__restrict__ dtx, mtcp_gpu_rto_rec *__restrict__ rec,
                                                       uint32_t *__restrict__ seg_sid, uint32_t *__restrict__ seg_start,
                                                       uint32_t *__restrict__ seg_stop, uint32_t *__restrict__ nseg,
                                                       uint64_t *__restrict__ total) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const uint32_t run = cnt[wave];
    const uint64_t *wb = ballots + (uint64_t)wave * kRtoRounds;
#pragma unroll
    for (int r = 0; r < kRtoRounds; ++r) {
        const uint64_t m = wb[r];
        const uint64_t id = (uint64_t)wave * kRtoWaveChunk + (uint32_t)r * kWave + lane;
        const uint64_t k = id >> shift;
        if (!((m >> lane) & 1ull) || id > P.max_id || k >= P.cap) continue;
        const uint64_t sa = (uint64_t)snd + 128ull * id;
        const v4u q0 = gload(sa), q1 = gload(sa + 16), q2 = gload(sa + 32), q3 = gload(sa + 48), q4 = gload(sa + 64);
        const v2u q5 = gload64(sa + 80);
        const v4u d = gload((uint64_t)dtx + 16ull * id);
        uint32_t *srec = reinterpret_cast<uint32_t *>(snd + 128ull * id);
        srec[0] = q0.x, srec[7] = q1.w, srec[8] = q2.x, srec[9] = q2.y, srec[20] = q5.x, srec[21] = q5.y;
        dtx[16ull * id + 12] = (uint8_t)d.w;
        const v4u rv = {(uint32_t)id, q0.y + q0.w + q2.w + q3.z, q4.y + q4.z + q4.w, run};
        *reinterpret_cast<gsv4u *>((uint64_t)rec + 16ull * k) = rv;
        seg_sid[k] = (uint32_t)id;
    }
    rto_table(blockIdx.x * kBlock + threadIdx.x, gridDim.x * kBlock, tot[0], P, seg_start, seg_stop, nseg, total);
}

}  // namespace

// mtcp_gpu_rto_sweep_dev's three launches with cond_count_kernel in the count
// kernel's place, whatever the sizes.  The arguments are the call's, unchecked.
// 0, or -1 on a launch error.
extern "C" int rtosweep_cond(uint32_t max_id, void *d_snd, void *d_dtx, uint32_t cur_ts, uint32_t cap, void *d_rto,
                             void *d_seg_sid, void *d_seg_start, void *d_seg_stop, void *d_nseg, void *d_total,
                             void *d_work, void *stream) {
    const RtoSweepWork w = rto_sweep_work(max_id);
    const RtoSweepParams P{max_id, cap, cur_ts};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    uint8_t *work = static_cast<uint8_t *>(d_work), *snd = static_cast<uint8_t *>(d_snd);
    const auto u32 = [](void *p) { return static_cast<uint32_t *>(p); };
    uint64_t *ballots = reinterpret_cast<uint64_t *>(work + w.ballot_off);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(work + w.cnt_off), *tot = reinterpret_cast<uint32_t *>(work + w.tot_off);
    hipLaunchKernelGGL(cond_count_kernel, dim3(w.ntiles), dim3(kBlock), 0, st, snd, P, ballots, cnt);
    hipLaunchKernelGGL(steer_scan_kernel, dim3(1), dim3(kBlock), 0, st, cnt, w.nwaves, tot);
    hipLaunchKernelGGL(rto_emit_kernel, dim3(w.ntiles), dim3(kBlock), 0, st, ballots, cnt, tot, P, snd,
                       static_cast<uint8_t *>(d_dtx), static_cast<mtcp_gpu_rto_rec *>(d_rto), u32(d_seg_sid),
                       u32(d_seg_start), u32(d_seg_stop), u32(d_nseg), static_cast<uint64_t *>(d_total));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The three-launch form's pattern: d_work as the sweep left it (its masks are
// read), d_scratch another workspace of the same size for what pattern_count
// stores.  0, or -1 on a launch error.
extern "C" int rtosweep_pattern(uint32_t max_id, void *d_snd, void *d_dtx, uint32_t cur_ts, uint32_t cap, uint32_t shift,
                                void *d_rto, void *d_seg_sid, void *d_seg_start, void *d_seg_stop, void *d_nseg,
                                void *d_total, void *d_work, void *d_scratch, void *stream) {
    const RtoSweepWork w = rto_sweep_work(max_id);
    const RtoSweepParams P{max_id, cap, cur_ts};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    uint8_t *work = static_cast<uint8_t *>(d_work), *scr = static_cast<uint8_t *>(d_scratch);
    const auto u32 = [](void *p) { return static_cast<uint32_t *>(p); };
    hipLaunchKernelGGL(pattern_count, dim3(w.ntiles), dim3(kBlock), 0, st, static_cast<const uint8_t *>(d_snd), P,
                       reinterpret_cast<uint64_t *>(scr + w.ballot_off), reinterpret_cast<uint32_t *>(scr + w.cnt_off));
    hipLaunchKernelGGL(steer_scan_kernel, dim3(1), dim3(kBlock), 0, st, reinterpret_cast<uint32_t *>(scr + w.cnt_off),
                       w.nwaves, reinterpret_cast<uint32_t *>(scr + w.tot_off));
    hipLaunchKernelGGL(pattern_emit, dim3(w.ntiles), dim3(kBlock), 0, st,
                       reinterpret_cast<const uint64_t *>(work + w.ballot_off),
                       reinterpret_cast<const uint32_t *>(work + w.cnt_off),
                       reinterpret_cast<const uint32_t *>(work + w.tot_off), P, shift, static_cast<uint8_t *>(d_snd),
                       static_cast<uint8_t *>(d_dtx), static_cast<mtcp_gpu_rto_rec *>(d_rto), u32(d_seg_sid),
                       u32(d_seg_start), u32(d_seg_stop), u32(d_nseg), static_cast<uint64_t *>(d_total));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
