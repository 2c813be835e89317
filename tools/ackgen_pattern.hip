// ackgen_pattern.hip — the memory pattern of the ACK generation
// (mtcp_amd/csrc/ackgen_kernels.hpp) without its arithmetic, and the library's
// three launches with the plan kernel's lane threshold as a parameter: the
// yardstick and the sweep of tools/ackgen_bench.py.  Measurement
// infrastructure: nothing here is part of libmtcp_gpu.so.
//
// The pattern: the same three launches on the same grids.  pattern_plan takes
// the segments as the plan kernel does (the lanes' own loops, then the wave
// over the long lists, 64 placement dwords a step), loads the same tx record,
// state pieces, snd_nxt, indices and placement dwords and stores the same 32 B
// plan, prefix and sums; what it stores is a sum of what it loaded: no fold,
// no BAD test, no to_ack, and the planned count is the record's own ack_cnt
// field, so that the emit has the same fan-out only where the caller passes
// tx records that already hold the counts (the bench tool does).  The scan has
// no arithmetic to leave out and is the library's kernel.  pattern_emit does
// the same two searches and loads, and stores the plan's words as the record,
// the descriptor, the void tail, the three dwords of the tx record and the
// result, without the record's or the commit's arithmetic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../mtcp_amd/csrc/ackgen_kernels.hpp"

namespace {

using namespace mg;

template <uint32_t LANE_MAX>
__global__ __launch_bounds__(kBlock) void pattern_plan(
    const uint8_t *__restrict__ place, const uint32_t *__restrict__ idx, const AckGenParams P,
    const uint32_t *__restrict__ seg_sid, const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ nseg,
    const uint32_t *__restrict__ seg_stop, const uint32_t *__restrict__ ack_stop, const uint8_t *__restrict__ state,
    const uint8_t *__restrict__ snd, const uint8_t *__restrict__ tx, v4u *__restrict__ plan,
    uint32_t *__restrict__ local, uint32_t *__restrict__ part_c, uint64_t *__restrict__ part_b) {
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
    v4u a = {0, 0, 0, 0}, b = {0, 0, 0, 0}, s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
    uint32_t snd_nxt = 0, stopc = start;
    if (is_stream) {
        a = gload((uint64_t)tx + 32ull * sid), b = gload((uint64_t)tx + 32ull * sid + 16);
        s0 = gload((uint64_t)state + 64ull * sid);
        s1 = gload((uint64_t)state + 64ull * sid + 16);
        snd_nxt = gload32((uint64_t)snd + 128ull * sid);
        stopc = min(max(seg_stop[j] + (ack_stop ? ack_stop[j] & 0u : 0u), start), end);
    }
    uint32_t f = 0;
    const bool lng = stopc - start > LANE_MAX;
    if (!lng) {
        for (uint32_t p = start; p < stopc; ++p) {
            const uint32_t q = idx[p];
            if (q >= n) continue;
            f += gload32((uint64_t)place + 16ull * q + 12);
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
                if (q < n) w = gload32((uint64_t)place + 16ull * q + 12);
            }
            lf += (uint32_t)__popcll(__ballot(w >> 31));           // one value out of the step's 64 loads
        }
        if ((int)lane == l) f = lf;
    }
    uint32_t c = 0;
    if (valid) {
        c = is_stream ? (a.w >> 16) & 63u : 0u;                    // the record's own count: the emit's fan-out
        const uint32_t meta = c | ((b.x >> 8) & 0xFFu) << 8 | (is_stream ? MTCP_GPU_ACKGEN_SENT : 0u) << 16;
        const v4u pa = {a.x, a.y, a.z, snd_nxt + f}, pb = {s0.x + s0.y + s0.z + s0.w, s1.y + s1.w + b.y, a.w & 0xFFFF0000u, meta};
        *reinterpret_cast<gsv4u *>((uint64_t)plan + 32ull * j) = pa;
        *reinterpret_cast<gsv4u *>((uint64_t)plan + 32ull * j + 16) = pb;
    }
    uint32_t ec, tc;
    uint64_t eb, tb;
    txseg_block_scan<kWavesPerBlock>(c < P.seg_cap ? c : P.seg_cap, 0ull, P.seg_cap, ec, eb, tc, tb);
    if (valid) local[j] = ec;
    if (threadIdx.x == 0) part_c[blockIdx.x] = tc, part_b[blockIdx.x] = 0ull;
}

__global__ __launch_bounds__(kBlock) void pattern_emit(
    const v4u *__restrict__ plan, const uint32_t *__restrict__ local, const uint32_t *__restrict__ part_c,
    const uint32_t *__restrict__ tot_c, const uint32_t *__restrict__ nseg, uint32_t nwg, const AckGenParams P,
    const uint32_t *__restrict__ seg_sid, uint8_t *__restrict__ tx, mtcp_gpu_tx_seg *__restrict__ seg,
    mtcp_gpu_desc *__restrict__ desc, mtcp_gpu_ackgen_res *__restrict__ ares, uint64_t *__restrict__ d_total) {
    const uint32_t m = min(nseg[0], P.n);
    const uint32_t T = min(*tot_c, P.room);
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k == 0) d_total[0] = T, d_total[1] = (uint64_t)T * P.slot;
    if (k < P.seg_cap) {
        if (k < T) {
            const uint32_t b = txseg_search(part_c, 0u, nwg - 1, k);
            const uint32_t lo = b * kBlock, hi = min(m, lo + kBlock) - 1, r = k - part_c[b];
            const uint32_t j = txseg_search(local, lo, hi, r);
            const v4u pa = gload((uint64_t)plan + 32ull * j), pb = gload((uint64_t)plan + 32ull * j + 16);
            const v4u e = {pb.z, pb.w, 0u, r - local[j]};
            const uint64_t at = (uint64_t)seg + 48ull * k;
            *reinterpret_cast<gsv4u *>(at) = pa;
            *reinterpret_cast<gsv4u *>(at + 16) = pb;
            *reinterpret_cast<gsv4u *>(at + 32) = e;
            const v2u d = {(uint32_t)((P.buf_off + (uint64_t)k * P.slot) >> P.off_shift), MTCP_GPU_ACKGEN_FRAME_LEN};
            *reinterpret_cast<gsv2u *>((uint64_t)desc + 8ull * k) = d;
        } else {
            txseg_store_void(seg, desc, k);
        }
    }
    if (k < m) {
        const v4u pa = gload((uint64_t)plan + 32ull * k), pb = gload((uint64_t)plan + 32ull * k + 16);
        const uint32_t S = part_c[k / kBlock] + local[k];
        const uint32_t sid = seg_sid[k];
        if (sid <= P.max_id) {
            uint32_t *rec = reinterpret_cast<uint32_t *>(tx + 32ull * sid);
            rec[3] = pb.z | (pb.w & 63u) << 16, rec[4] = pa.w, rec[5] = pb.y;
        }
        const v4u rv = {S, pb.w, pb.x, pb.z};
        *reinterpret_cast<gsv4u *>((uint64_t)ares + 16ull * k) = rv;
    }
}

struct Args {
    AckGenParams P;
    AckGenWork w;
    v4u *plan;
    uint32_t *local, *part_c, *tot_c;
    uint64_t *part_b;
    unsigned long long *tot_b;
};
Args args_of(uint32_t n, uint32_t max_id, uint32_t seg_cap, void *d_work) {
    Args a{};
    a.P.n = n, a.P.max_id = max_id, a.P.n_links = 256, a.P.cur_ts = 0x12345678u, a.P.off_shift = 6;
    a.P.slot = 128, a.P.seg_cap = seg_cap, a.P.room = seg_cap;
    a.w = ackgen_work(n);
    uint8_t *work = static_cast<uint8_t *>(d_work);
    a.plan = reinterpret_cast<v4u *>(work + a.w.plan_off);
    a.local = reinterpret_cast<uint32_t *>(work + a.w.local_off);
    a.part_c = reinterpret_cast<uint32_t *>(work + a.w.pc_off);
    a.part_b = reinterpret_cast<uint64_t *>(work + a.w.pb_off);
    a.tot_b = reinterpret_cast<unsigned long long *>(work + a.w.tot_off);
    a.tot_c = reinterpret_cast<uint32_t *>(work + a.w.tot_off + 8);
    return a;
}

template <uint32_t LANE_MAX, bool PATTERN>
int launch(const void *d_place, uint32_t n, uint32_t max_id, const void *d_idx, const void *d_seg_sid,
           const void *d_seg_start, const void *d_nseg, const void *d_seg_stop, const void *d_ack_stop,
           const void *d_state, const void *d_snd, void *d_tx, void *d_seg, void *d_desc, uint32_t seg_cap,
           void *d_ares, void *d_total, void *d_work, void *stream) {
    if (!n || !seg_cap) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const Args a = args_of(n, max_id, seg_cap, d_work);
    const dim3 block(kBlock);
    const auto u8 = [](const void *p) { return static_cast<const uint8_t *>(p); };
    const auto u32 = [](const void *p) { return static_cast<const uint32_t *>(p); };
    if (PATTERN)
        hipLaunchKernelGGL(pattern_plan<LANE_MAX>, dim3(a.w.nwg), block, 0, st, u8(d_place), u32(d_idx), a.P, u32(d_seg_sid),
                           u32(d_seg_start), u32(d_nseg), u32(d_seg_stop), u32(d_ack_stop), u8(d_state), u8(d_snd),
                           u8(d_tx), a.plan, a.local, a.part_c, a.part_b);
    else
        hipLaunchKernelGGL(ackgen_plan_kernel<LANE_MAX>, dim3(a.w.nwg), block, 0, st, u8(d_place), u32(d_idx), a.P,
                           u32(d_seg_sid), u32(d_seg_start), u32(d_nseg), u32(d_seg_stop), u32(d_ack_stop), u8(d_state),
                           u8(d_snd), u8(d_tx), a.plan, a.local, a.part_c, a.part_b);
    hipLaunchKernelGGL(txseg_scan_kernel, dim3(1), block, 0, st, a.part_c, a.part_b, a.w.nwg, seg_cap, a.tot_c, a.tot_b);
    const uint32_t lanes = seg_cap > n ? seg_cap : n;
    const dim3 grid((lanes + kBlock - 1) / kBlock);
    if (PATTERN)
        hipLaunchKernelGGL(pattern_emit, grid, block, 0, st, a.plan, a.local, a.part_c, a.tot_c, u32(d_nseg), a.w.nwg, a.P,
                           u32(d_seg_sid), static_cast<uint8_t *>(d_tx), static_cast<mtcp_gpu_tx_seg *>(d_seg),
                           static_cast<mtcp_gpu_desc *>(d_desc), static_cast<mtcp_gpu_ackgen_res *>(d_ares),
                           static_cast<uint64_t *>(d_total));
    else
        hipLaunchKernelGGL(ackgen_emit_kernel, grid, block, 0, st, a.plan, a.local, a.part_c, a.tot_c, u32(d_nseg), a.w.nwg,
                           a.P, u32(d_seg_sid), static_cast<uint8_t *>(d_tx), static_cast<mtcp_gpu_tx_seg *>(d_seg),
                           static_cast<mtcp_gpu_desc *>(d_desc), static_cast<mtcp_gpu_ackgen_res *>(d_ares),
                           static_cast<uint64_t *>(d_total));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace

// The pattern for a grouped batch, on `stream`: the arguments of
// mtcp_gpu_ackgen_dev with 128 B slots from offset 0, a shift of 6 and room
// for all seg_cap records; d_work as mtcp_gpu_ackgen_work_bytes sizes it.
// d_tx[id].ack_cnt is the stream's fan-out.  0, or -1 on a launch error.
extern "C" int ackgen_pattern_launch(const void *d_place, uint32_t n, uint32_t max_id, const void *d_idx,
                                     const void *d_seg_sid, const void *d_seg_start, const void *d_nseg,
                                     const void *d_seg_stop, const void *d_ack_stop, const void *d_state,
                                     const void *d_snd, void *d_tx, void *d_seg, void *d_desc, uint32_t seg_cap,
                                     void *d_ares, void *d_total, void *d_work, void *stream) {
    return launch<kAckgenLaneMax, true>(d_place, n, max_id, d_idx, d_seg_sid, d_seg_start, d_nseg, d_seg_stop, d_ack_stop,
                                        d_state, d_snd, d_tx, d_seg, d_desc, seg_cap, d_ares, d_total, d_work, stream);
}

// The library's three launches with the plan kernel's lane threshold
// lane_max (4, 8, 16, 32, 64 or 128), same arguments.  -2 for another value.
extern "C" int ackgen_variant_launch(uint32_t lane_max, const void *d_place, uint32_t n, uint32_t max_id,
                                     const void *d_idx, const void *d_seg_sid, const void *d_seg_start,
                                     const void *d_nseg, const void *d_seg_stop, const void *d_ack_stop,
                                     const void *d_state, const void *d_snd, void *d_tx, void *d_seg, void *d_desc,
                                     uint32_t seg_cap, void *d_ares, void *d_total, void *d_work, void *stream) {
#define VARIANT(L)                                                                                                      \
    if (lane_max == L)                                                                                                  \
        return launch<L, false>(d_place, n, max_id, d_idx, d_seg_sid, d_seg_start, d_nseg, d_seg_stop, d_ack_stop,      \
                                d_state, d_snd, d_tx, d_seg, d_desc, seg_cap, d_ares, d_total, d_work, stream);
    VARIANT(4) VARIANT(8) VARIANT(16) VARIANT(32) VARIANT(64) VARIANT(128)
#undef VARIANT
    return -2;
}
