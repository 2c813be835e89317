// rcvread_kernels.hpp — gfx950 kernels of the batched application read out of
// device receive buffers: CopyToUser / PeekForUser
// (mtcp/src/api.c:1096-1149) and RBRemove (mtcp/src/tcp_ring_buffer.c:384-421)
// for a batch of read requests.  include/mtcp_gpu_rcvread.h has the contract,
// rcvread_step.hpp the step.
//
// Five launches, ordered by the stream:
//
//   clear   a lane per request: "none" to the claim word of the request's sid
//           (the workspace is never cleared as a whole); lane 0 zeroes d_total;
//   claim   a lane per request: an agent-scope atomic minimum of the request
//           index into the claim word of its sid.  No lane waits for another;
//   plan    a lane per request: the request is DUP if the claim word is not its
//           index; read_step gives the verdict, the new records and the result
//           record, which the lane stores; the copy's source, destination and
//           length go to the request's plan row, the number of its copy units
//           through a block scan to cnt[] (the prefix inside the workgroup) and
//           part[] (the workgroup's units); the wave's copied requests and
//           bytes are added to d_total (integer adds: any order gives the sum);
//   scan    steer_scan_kernel (steer_kernels.hpp), ONE workgroup: the exclusive
//           prefix of part[], the total = the batch's units;
//   copy    the hot path.  A wave per unit, the grid walking the units with its
//           stride: the unit's request by binary search in part[] and then in
//           the 256 entries of cnt[] of that workgroup; kReadUnitChunks pieces
//           of the destination's 16 B grid, four a lane; every piece's two
//           source loads (non-temporal: a run is read once) are issued before
//           the first store; the source is funnel-shifted to the destination's
//           alignment (read_chunk_value, as rcvcopy_kernels.hpp's copy_run does
//           it) and stored with one 16 B store per inner piece, dword, short
//           and byte stores at the run's two edges (read_chunk_store).
//
// A 1 MiB run is 256 or 257 units and keeps as many waves busy; a 1-byte run
// is one unit whose wave issues one load and one byte store.
//
// What the copy stores is decided by one plan lane from the records it loaded
// and handed over as two 16 B rows: the stores stay inside [dst_off, dst_off +
// copylen) of an accepted request for any bytes in the records.  No workgroup
// waits on another, no LDS beyond the block scan's, no scratch; every loop's
// trip count is fixed by n, the unit size or a record's clamped size.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu_rcvread.h"
#include "rcvcopy_kernels.hpp"   // copy_piece, the gs* store types; kWave, kBlock, gload through rx_kernels.hpp
#include "rcvread_step.hpp"
#include "steer_kernels.hpp"     // steer_scan_kernel, block_exclusive_scan

namespace mg {

constexpr uint32_t kReadNone = 0xFFFFFFFFu;
constexpr int kReadRounds = kReadUnitChunks / kWave;              // pieces a lane moves per unit
static_assert(kReadUnitChunks % kWave == 0, "a unit is whole rounds of a wave");

// The workspace: the claim word of every stream id, then per request its unit
// prefix inside its workgroup and its two plan rows, per plan workgroup its
// units (scanned in place), the total.
struct ReadWork {
    uint32_t nwg;
    uint64_t claim_off, cnt_off, part_off, tot_off, plan_off, bytes;
};
inline ReadWork read_work(uint32_t n, uint32_t max_id) {
    ReadWork w{};
    w.nwg = (uint32_t)(((uint64_t)(n ? n : 1) + kBlock - 1) / kBlock);
    w.claim_off = 0;
    w.cnt_off = (4ull * ((uint64_t)max_id + 1) + 15) & ~15ull;
    w.part_off = w.cnt_off + 4ull * kBlock * w.nwg;
    w.tot_off = w.part_off + ((4ull * w.nwg + 15) & ~15ull);
    w.plan_off = w.tot_off + 16;
    w.bytes = w.plan_off + 32ull * kBlock * w.nwg;
    return w;
}

struct ReadParams {
    uint32_t n, max_id;
    uint64_t arena_bytes, dst_bytes;
};

// ---- clear --------------------------------------------------------------------
// grid: one lane per request.
__global__ __launch_bounds__(kBlock) void rcvread_clear_kernel(const uint4 *__restrict__ req, const ReadParams P,
                                                               uint32_t *__restrict__ claim,
                                                               uint64_t *__restrict__ total) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) total[0] = 0, total[1] = 0;
    if (i >= P.n) return;
    const uint32_t sid = req[2ull * i].x;
    if (sid <= P.max_id) claim[sid] = kReadNone;
}

// ---- claim --------------------------------------------------------------------
// grid: one lane per request.
__global__ __launch_bounds__(kBlock) void rcvread_claim_kernel(const uint4 *__restrict__ req, const ReadParams P,
                                                               uint32_t *__restrict__ claim) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t sid = req[2ull * i].x;
    if (sid <= P.max_id) atomicMin(&claim[sid], i);
}

// ---- plan ---------------------------------------------------------------------
// grid: one lane per request, whole workgroups.  pack: where the request's
// bytes go instead of dst_off (the synchronous form's gather), or nullptr.
__global__ __launch_bounds__(kBlock) void rcvread_plan_kernel(const uint4 *__restrict__ req, const ReadParams P,
                                                              const uint32_t *__restrict__ claim, uint4 *state,
                                                              uint32_t *rbuf, uint8_t *tx,
                                                              const uint8_t *__restrict__ snd,
                                                              const uint64_t *__restrict__ pack,
                                                              uint4 *__restrict__ rres, uint64_t *total,
                                                              uint32_t *__restrict__ cnt, uint32_t *__restrict__ part,
                                                              uint4 *__restrict__ plan) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    uint32_t units = 0, copylen = 0;
    uint64_t src = 0, dst = 0;
    if (i < P.n) {
        ReadIn in{};
        const uint4 r0 = req[2ull * i], r1 = req[2ull * i + 1];
        in.req[0] = r0.x, in.req[1] = r0.y, in.req[2] = r0.z, in.req[3] = r0.w;
        in.req[4] = r1.x, in.req[5] = r1.y, in.req[6] = r1.z, in.req[7] = r1.w;
        in.max_id = P.max_id, in.arena_bytes = P.arena_bytes, in.dst_bytes = P.dst_bytes;
        const uint32_t sid = r0.x;
        if (sid <= P.max_id) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 v = state[4ull * sid + q];
                in.st[4 * q] = v.x, in.st[4 * q + 1] = v.y, in.st[4 * q + 2] = v.z, in.st[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const uint4 v = reinterpret_cast<const uint4 *>(rbuf)[2ull * sid + q];
                in.rb[4 * q] = v.x, in.rb[4 * q + 1] = v.y, in.rb[4 * q + 2] = v.z, in.rb[4 * q + 3] = v.w;
            }
            in.has_tx = tx != nullptr;
            if (in.has_tx) {
                in.need_wnd_adv = tx[32ull * sid + 19];
                in.eff_mss = *reinterpret_cast<const uint16_t *>(snd + 128ull * sid + 78);
            }
            // A request that lost its claim loads these records in the launch in which the winner stores
            // them.  Of what it loaded read_step looks at rb[2] (size) alone before it answers DUP, and no
            // READ changes size: a rule placed in front of DUP must not read a field a READ writes.
            in.dup = claim[sid] != i;
        }
        const ReadOut o = read_step(in);
        if (o.st_rec) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                state[4ull * sid + q] = make_uint4(o.st[4 * q], o.st[4 * q + 1], o.st[4 * q + 2], o.st[4 * q + 3]);
            rbuf[8ull * sid + 3] = o.rb_head, rbuf[8ull * sid + 5] = o.rb_last;
        }
        if (o.st_tx) tx[32ull * sid + 19] = 0;
        rres[i] = make_uint4(o.res[0], o.res[1], o.res[2], o.res[3]);
        copylen = o.copylen, src = o.src;
        dst = pack ? pack[i] : ((uint64_t)r0.w << 32 | r0.z);
        units = read_units(dst, copylen);
    }
    uint32_t excl;
    const uint32_t all = block_exclusive_scan(units, excl);
    cnt[i] = excl;                                                  // the workspace holds whole workgroups
    plan[2ull * i] = make_uint4((uint32_t)src, (uint32_t)(src >> 32), (uint32_t)dst, (uint32_t)(dst >> 32));
    plan[2ull * i + 1] = make_uint4(copylen, units, 0u, 0u);
    if (threadIdx.x == 0) part[blockIdx.x] = all;
    // the wave's share of d_total
    const uint64_t m = __ballot(copylen != 0);
    if (m) {                                                        // the same in every lane of the wave
        unsigned long long b = copylen;
#pragma unroll
        for (int d = kWave / 2; d >= 1; d >>= 1) b += __shfl_down(b, d, kWave);
        if ((threadIdx.x & (kWave - 1)) == 0) {
            atomicAdd(reinterpret_cast<unsigned long long *>(total), (unsigned long long)__popcll(m));
            atomicAdd(reinterpret_cast<unsigned long long *>(total) + 1, b);
        }
    }
}

// ---- copy ---------------------------------------------------------------------
// A chunk's value and its store: the body of rcvcopy_kernels.hpp's copy_run cut
// in two, because a unit issues every load before its first store.  copy_run
// itself keeps its text: f12's kernels are not rebuilt differently for this row.
// The 16 B of a destination chunk out of the two aligned source pieces that
// hold its bytes: sh = (src - dst) & 15 is the byte shift between the two grids.
__device__ __forceinline__ void read_chunk_value(const v4u &lo, const v4u &hi, uint32_t sh, uint32_t (&o)[4]) {
    const uint32_t k = sh >> 2, b = sh & 3u;
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t t[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) t[i] = k == 0 ? w[i] : k == 1 ? w[i + 1] : k == 2 ? w[i + 2] : w[i + 3];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = __builtin_amdgcn_alignbyte(t[i + 1], t[i], b);
}

// The bytes of the aligned chunk at byte d of `base` that lie inside [dst,
// dend): one 16 B store for an inner chunk; dword, short and byte stores at a
// run's two edges, so that no byte outside the run is written.
__device__ __forceinline__ void read_chunk_store(uint64_t base, uint64_t d, uint64_t dst, uint64_t dend,
                                                 const uint32_t (&o)[4]) {
    const uint32_t from = d < dst ? (uint32_t)(dst - d) : 0u, to = d + 16 > dend ? (uint32_t)(dend - d) : 16u;
    if (from == 0 && to == 16) {
        const v4u v = {o[0], o[1], o[2], o[3]};
        *reinterpret_cast<gsv4u *>(base + d) = v;
        return;
    }
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t at = 4 * i;
        if (from <= at && at + 4 <= to) {
            *reinterpret_cast<gsu32 *>(base + d + at) = o[i];
            continue;
        }
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t ah = at + 2 * h, v = o[i] >> (16 * h);
            if (from <= ah && ah + 2 <= to) {
                *reinterpret_cast<gsu16 *>(base + d + ah) = (uint16_t)v;
                continue;
            }
            if (from <= ah && ah + 1 <= to) *reinterpret_cast<gsu8 *>(base + d + ah) = (uint8_t)v;
            if (from <= ah + 1 && ah + 2 <= to) *reinterpret_cast<gsu8 *>(base + d + ah + 1) = (uint8_t)(v >> 8);
        }
    }
}

// The largest k < len with a[k] <= u; a is non-decreasing and a[0] <= u.
__device__ __forceinline__ uint32_t read_search(const uint32_t *__restrict__ a, uint32_t len, uint32_t u) {
    uint32_t lo = 0, hi = len;                                      // a[lo] <= u < a[hi] (a[len] = infinity)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= u) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Unit lu of the copy of len bytes from byte src of sbase to byte dst of dbase
// (both bases 16 B aligned), by one wave.
__device__ __forceinline__ void read_unit(uint64_t dbase, uint64_t dst, uint64_t sbase, uint64_t src, uint32_t len,
                                          uint32_t lu, uint32_t lane) {
    const uint64_t d0 = dst & ~15ull, dend = dst + len;
    const uint64_t nch = ((dend + 15) >> 4) - (dst >> 4);
    const int64_t slo = (int64_t)src, shi = (int64_t)(src + len);
    const uint32_t sh = (uint32_t)(src - dst) & 15u;
    const uint64_t c0 = (uint64_t)lu * kReadUnitChunks + lane;
    v4u lo[kReadRounds], hi[kReadRounds];
#pragma unroll
    for (int k = 0; k < kReadRounds; ++k) {
        const uint64_t c = c0 + (uint32_t)k * kWave;
        lo[k] = v4u{0u, 0u, 0u, 0u}, hi[k] = lo[k];
        if (c < nch) {
            const uint64_t d = d0 + 16ull * c;
            const int64_t a = slo + ((int64_t)d - (int64_t)dst) - (int64_t)sh;   // the aligned piece that holds d's byte
            lo[k] = copy_piece<true, false>(sbase, a, slo, shi, 0);
            if (sh) hi[k] = copy_piece<true, false>(sbase, a + 16, slo, shi, 0);  // aligned grids: the chunk is lo
        }
    }
#pragma unroll
    for (int k = 0; k < kReadRounds; ++k) {
        const uint64_t c = c0 + (uint32_t)k * kWave;
        if (c < nch) {
            uint32_t o[4];
            read_chunk_value(lo[k], hi[k], sh, o);
            read_chunk_store(dbase, d0 + 16ull * c, dst, dend, o);
        }
    }
}

// grid: any number of whole workgroups; wave w takes units w, w + waves, ...
__global__ __launch_bounds__(kBlock) void rcvread_copy_kernel(const uint32_t *__restrict__ cnt,
                                                              const uint32_t *__restrict__ part,
                                                              const uint32_t *__restrict__ tot, uint32_t nwg,
                                                              const uint4 *__restrict__ plan, uint64_t arena,
                                                              uint64_t dbase) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + threadIdx.x / kWave));
    const uint32_t waves = gridDim.x * kWavesPerBlock, total = tot[0];
    for (uint32_t u = wave; u < total; u += waves) {
        const uint32_t g = read_search(part, nwg, u);
        const uint32_t rel = u - part[g];
        const uint32_t j = read_search(cnt + (uint64_t)g * kBlock, kBlock, rel);
        const uint64_t i = (uint64_t)g * kBlock + j;
        const uint4 a = plan[2 * i], b = plan[2 * i + 1];
        const uint32_t lu = rel - cnt[i];
        // Not a unit of this request: nothing is stored.  The counts are uint32_t sums; with overlapping accepted
        // ranges they can wrap and the search can land anywhere, and this test then keeps every store a real
        // unit of a real request (the header's "with overlapping ranges the stores only stay bounded").
        if (lu >= b.y) continue;
        read_unit(dbase, (uint64_t)a.w << 32 | a.z, arena, (uint64_t)a.y << 32 | a.x, b.x, lu, lane);
    }
}

}  // namespace mg
