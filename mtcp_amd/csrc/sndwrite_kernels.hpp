// sndwrite_kernels.hpp — gfx950 kernels of the batched application write into
// device send buffers: mtcp_write's body, CopyFromUser
// (mtcp/src/api.c:1416-1567) and SBPut (mtcp/src/tcp_send_buffer.c:116-146) for
// a batch of write requests.  include/mtcp_gpu_sndwrite.h has the contract,
// sndwrite_step.hpp the step.
//
// Six launches, ordered by the stream:
//
//   clear   rcvread_clear_kernel (rcvread_kernels.hpp), unchanged: a request
//   claim   rcvread_claim_kernel, unchanged     begins with its sid in both rows;
//   plan    a lane per request: the request is DUP if the claim word is not its
//           index; write_step gives the verdict, the new record words and the
//           result record, which the lane stores with the request's table
//           entries; the copy's source, destination and length and the move's
//           length and distance go to the request's plan row, the number of its
//           copy units through a block scan to cnt[] and part[]; the wave's
//           written requests and bytes are added to d_total once per wave;
//   scan    steer_scan_kernel (steer_kernels.hpp), ONE workgroup;
//   move    SBPut's memmove (:136) for the compacting requests, before any byte
//           of the batch is copied: the copy's destination [sb_len, sb_len +
//           to_put) may overlap the old window [head_off, head_off + sb_len).  A
//           wave per request, which leaves at once unless plan gave the request
//           a move; rcvcopy_kernels.hpp's copy_run: ascending passes of 64
//           pieces, every lane's loads of a pass issued before any store, exact
//           stores at the two edges;
//   copy    the hot path.  A wave per 4 KiB unit of the destination's 16 B grid,
//           the unit's request by row f17's two-level search (read_search),
//           the unit itself by row f17's read_unit: both source pieces of every
//           16 B piece loaded (non-temporal: a user buffer is read once) before
//           the first store, the funnel shift to the destination's alignment,
//           one plain 16 B store per inner piece (row f7 reads the chunk next),
//           dword, short and byte stores at the run's edges.
//
// What move and copy store is decided by one plan lane from the records it
// loaded and handed over as two 16 B rows: the stores stay inside the chunk of
// a WRITTEN request for any bytes in the records.  No workgroup waits on
// another, no LDS beyond the block scan's, no scratch; every loop's trip count
// is fixed by n, the unit size or a record's clamped size.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu_sndwrite.h"
#include "rcvcopy_kernels.hpp"   // copy_run, copy_piece, the gs* store types
#include "rcvread_kernels.hpp"   // the claim kernels, ReadWork, read_search, read_unit
#include "sndwrite_step.hpp"
#include "steer_kernels.hpp"     // steer_scan_kernel, block_exclusive_scan

namespace mg {

static_assert(kWriteUnit == kReadUnit, "read_unit moves one unit of row f17's size");

struct WriteParams {
    uint32_t n, max_id;
    uint64_t src_bytes, payload_bytes;
};

// ---- plan ---------------------------------------------------------------------
// grid: one lane per request, whole workgroups.  pack: where the request's
// bytes lie instead of src_off (the synchronous form's packing), or nullptr.
__global__ __launch_bounds__(kBlock) void sndwrite_plan_kernel(
    const uint4 *__restrict__ req, const WriteParams P, const uint32_t *__restrict__ claim, uint32_t *snd, uint32_t *dtx,
    const uint64_t *__restrict__ pack, uint4 *__restrict__ wres, uint32_t *__restrict__ seg_sid,
    uint32_t *__restrict__ seg_start, uint32_t *__restrict__ seg_stop, uint32_t *__restrict__ nseg, uint64_t *total,
    uint32_t *__restrict__ cnt, uint32_t *__restrict__ part, uint4 *__restrict__ plan) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    uint32_t units = 0, to_put = 0, move_len = 0, head_off = 0;
    uint64_t src = 0, dst = 0;
    if (i < P.n) {
        WriteIn in{};
        const uint4 r0 = req[2ull * i], r1 = req[2ull * i + 1];
        in.req[0] = r0.x, in.req[1] = r0.y, in.req[2] = r0.z, in.req[3] = r0.w;
        in.req[4] = r1.x, in.req[5] = r1.y, in.req[6] = r1.z, in.req[7] = r1.w;
        in.max_id = P.max_id, in.src_bytes = P.src_bytes, in.payload_bytes = P.payload_bytes;
        const uint32_t sid = r0.x;
        if (sid <= P.max_id) {
            uint32_t *s = snd + 32ull * sid, *d = dtx + 4ull * sid;
            in.snd_wnd = s[2];
            const uint4 v = reinterpret_cast<const uint4 *>(s)[4];          // dwords 16-19
            in.sb_head_seq = v.x, in.sb_len = v.y, in.sb_size = v.z, in.mss2 = v.w;
            in.bits = s[20], in.bits2 = s[21];
            const uint4 w = *reinterpret_cast<const uint4 *>(d);
            in.sb_off = (uint64_t)w.y << 32 | w.x, in.sb_base_seq = w.z, in.dflags = w.w;
            // A request that lost its claim loads these records in the launch in which the winner stores
            // them: write_step looks at none of them before it answers DUP.
            in.dup = claim[sid] != i;
        }
        const WriteOut o = write_step(in);
        if (o.st_wnd) snd[32ull * sid + 2] = o.snd_wnd;
        if (o.st_rec) {
            snd[32ull * sid + 17] = o.sb_len;
            dtx[4ull * sid + 2] = o.sb_base_seq;
            reinterpret_cast<uint8_t *>(dtx)[16ull * sid + 12] = 1;
        }
        wres[i] = make_uint4(o.res[0], o.res[1], o.res[2], o.res[3]);
        // the table row f15 takes: every list empty, the stream only where it was written
        seg_sid[i] = o.st_rec ? sid : MTCP_GPU_FLOW_NONE;
        seg_start[i] = 0, seg_stop[i] = 0;
        if (i == 0) seg_start[P.n] = 0, nseg[0] = P.n;
        to_put = o.to_put, dst = o.dst, move_len = o.move_len, head_off = o.head_off;
        src = pack ? pack[i] : o.src;
        units = write_units(dst, to_put);
    }
    uint32_t excl;
    const uint32_t all = block_exclusive_scan(units, excl);
    cnt[i] = excl;                                                  // the workspace holds whole workgroups
    plan[2ull * i] = make_uint4((uint32_t)src, (uint32_t)(src >> 32), (uint32_t)dst, (uint32_t)(dst >> 32));
    plan[2ull * i + 1] = make_uint4(to_put, units, move_len, head_off);
    if (threadIdx.x == 0) part[blockIdx.x] = all;
    // the wave's share of d_total
    const uint64_t m = __ballot(to_put != 0);
    if (m) {                                                        // the same in every lane of the wave
        unsigned long long b = to_put;
#pragma unroll
        for (int d = kWave / 2; d >= 1; d >>= 1) b += __shfl_down(b, d, kWave);
        if ((threadIdx.x & (kWave - 1)) == 0) {
            atomicAdd(reinterpret_cast<unsigned long long *>(total), (unsigned long long)__popcll(m));
            atomicAdd(reinterpret_cast<unsigned long long *>(total) + 1, b);
        }
    }
}

// ---- move ---------------------------------------------------------------------
// grid: one wave per request, whole workgroups.  The window of a compacting
// request moves down by head_off >= 1 to the chunk's first byte, which lies
// sb_len (= move_len) below the copy's destination.
__global__ __launch_bounds__(kBlock) void sndwrite_move_kernel(const uint4 *__restrict__ plan, uint32_t n,
                                                               uint64_t arena) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + threadIdx.x / kWave));
    if (i >= n) return;
    const uint4 b = plan[2ull * i + 1];
    if (b.z == 0) return;                                           // the whole wave
    const uint4 a = plan[2ull * i];
    const uint64_t to = ((uint64_t)a.w << 32 | a.z) - b.z;
    copy_run<(int)kWave, false, false>(arena, to, arena, to + b.w, b.z, lane, 0);
}

// ---- copy ---------------------------------------------------------------------
// grid: any number of whole workgroups; wave w takes units w, w + waves, ...
__global__ __launch_bounds__(kBlock) void sndwrite_copy_kernel(const uint32_t *__restrict__ cnt,
                                                               const uint32_t *__restrict__ part,
                                                               const uint32_t *__restrict__ tot, uint32_t nwg,
                                                               const uint4 *__restrict__ plan, uint64_t sbase,
                                                               uint64_t arena) {
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
        // Not a unit of this request: nothing is stored.  The counts are uint32_t sums; with overlapping chunks
        // they can wrap and the search can land anywhere, and this test then keeps every store a real unit of a
        // real request.
        if (lu >= b.y) continue;
        read_unit(arena, (uint64_t)a.w << 32 | a.z, sbase, (uint64_t)a.y << 32 | a.x, b.x, lu, lane);
    }
}

}  // namespace mg
