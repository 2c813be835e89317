// rcvcopy_kernels.hpp — gfx950 kernels of the payload copy behind the receive
// walk: RBPut's byte work, mtcp/src/tcp_ring_buffer.c:304-319
// (the compaction, the memcpy to head + putx, the tail_offset / last_len
// update), for every packet rcvwalk_kernels.hpp marked MTCP_GPU_RCV_COPY.
// include/mtcp_gpu_rcvcopy.h has the contract and the argument for the order.
//
// Four launches, ordered by the stream:
//
//   prep     one lane per position j of d_idx: the source tests of packet
//            d_idx[j] (payload_len, the payload inside the descriptor, the
//            descriptor inside the chunk) and its 16 B copy input {source byte
//            offset, put_off, put_len | code} to position j of the workspace,
//            so that a planner reads a list as one contiguous run; the
//            position's plan word cleared; d_cstat[j] = 0, so that every status
//            byte is written whatever the lists hold;
//   plan     one lane per segment, 64 consecutive segments a wave.  A lane
//            walks its list to seg_stop with one independent 16 B load per
//            step: the copyable tests, M, the class of every packet, whether
//            :304 fires.  A list longer than MTCP_GPU_RCVCOPY_WAVE_LEN is left
//            to the whole wave, 64 packets a step: a prefix maximum with a
//            carry gives every M, a ballot the trigger.  Then the wave moves
//            the window of each of its compacting streams (below), one after
//            the other, and the lanes write the new records and the segment
//            summaries;
//   front    G lanes per position, every FRONT packet of every stream at once:
//            the hot path;
//   ordered  one lane per segment again, the wave taking the segments that
//            have ORDERED packets one after the other and each packet with all
//            64 lanes, a fence between two packets.
//
// The copy (copy_run) cuts the destination on its absolute 16 B grid.  A chunk
// comes from the two aligned 16 B source pieces that hold its bytes (the
// second one is the next lane's first and comes from the same cache line) and
// a byte funnel shift that is constant per packet; one aligned 16 B store per
// inner chunk; dword, short and byte stores only in a packet's first and last
// chunk.  A piece is loaded only if it holds a byte of the source run.
//
// Compaction moves last_len bytes down by head_offset >= 1, ascending, a pass
// of 64 chunks at a time.  Pass k stores to the window's bytes
// [1024 k - e, 1024 (k + 1) - e) (e < 16: the grid's offset) and every later
// pass takes its bytes from positions at least head_offset above the highest
// byte stored so far, so no later pass needs a byte an earlier pass has
// overwritten; a piece it loads may hold such bytes, the funnel shift drops
// them.  Within a pass every lane's loads are issued before any lane's store
// (one wave, one instruction stream; the store waits for the loaded data).
//
// What a copy kernel stores is decided by one plan lane from one 16 B load of
// the buffer record and the immutable copy inputs, and handed over as single
// 8 B and 16 B words: the stores stay inside the record's chunk for any group
// arrays.  No workgroup waits on another, no atomic, no LDS; every loop's trip
// count is fixed by n, a list length or a payload length.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu.h"
#include "../../include/mtcp_gpu_rcvcopy.h"
#include "rx_kernels.hpp"        // kWave, kBlock, gload, gload_nt

namespace mg {

constexpr uint32_t kCopyWaveLen = MTCP_GPU_RCVCOPY_WAVE_LEN;
constexpr uint32_t kCopyCodeOk = 0x40, kCopyCodeBadSrc = 0x80;   // prep's codes: never a class
constexpr uint32_t kCopyCopyable = 0xFFu;

struct CopyWork {
    uint64_t in_off, plan_off, sum_off, bytes;
};
inline CopyWork copy_work(uint32_t n) {
    const uint64_t k = n ? n : 1;
    CopyWork w{};
    w.in_off = 0;                  // uint4 per position: src lo, src hi, put_off, put_len | code << 16
    w.plan_off = 16 * k;           // uint2 per position: segment, class
    w.sum_off = w.plan_off + ((8 * k + 15) & ~15ull);   // uint4 per segment: base lo, base hi, ORDERED packets, compacts
    w.bytes = w.sum_off + 16 * k;
    return w;
}

__host__ __device__ __forceinline__ uint32_t copy_umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// One mtcp_gpu_rcv_buf in registers.
struct CopyBuf {
    uint64_t data_off;
    uint32_t size, head, tail, last, r0, r1;
};
__host__ __device__ __forceinline__ bool copy_buf_bad(const CopyBuf &b, uint64_t arena_bytes) {
    return (b.r0 | b.r1) != 0 || b.size == 0 || b.size > MTCP_GPU_RCV_MAX_SIZE || b.data_off > arena_bytes ||
           b.size > arena_bytes - b.data_off || b.head > b.tail || b.tail > b.size || b.last != b.tail - b.head;
}

// The source tests of one packet.  place_w: the placement record's last word;
// res_w8: the result record's word at byte 32 (payload_len | ihl_doff << 16 |
// tcp_flags << 24).  Returns the code; src: the payload's byte offset in the chunk.
__host__ __device__ __forceinline__ uint32_t copy_src(uint32_t place_w, uint32_t res_w8, uint32_t desc_off,
                                                      uint32_t desc_len, uint32_t off_shift, uint64_t buf_len,
                                                      uint64_t &src) {
    src = 0;
    if (!((place_w >> 24) & MTCP_GPU_RCV_COPY)) return 0;
    const uint32_t put_len = place_w & 0xFFFFu, ihl_doff = (res_w8 >> 16) & 0xFFu;
    const uint32_t hdr = 14 + 4 * ((ihl_doff & 15u) + (ihl_doff >> 4));
    const uint64_t at = (uint64_t)desc_off << off_shift;
    if ((res_w8 & 0xFFFFu) != put_len || hdr + put_len > desc_len || at + desc_len > buf_len) return kCopyCodeBadSrc;
    src = at + hdr;
    return kCopyCodeOk;
}

// The class of one packet, but for FRONT / ORDERED: kCopyCopyable for a copyable one.
__host__ __device__ __forceinline__ uint32_t copy_class(bool bad, uint32_t size, uint32_t put_off, uint32_t len,
                                                        uint32_t code) {
    if (code == 0) return MTCP_GPU_RCVCOPY_NONE;
    if (bad) return MTCP_GPU_RCVCOPY_BAD_BUF;
    if ((uint64_t)put_off + len > size) return MTCP_GPU_RCVCOPY_BAD_RANGE;
    if (code != kCopyCodeOk) return MTCP_GPU_RCVCOPY_BAD_SRC;
    return kCopyCopyable;
}

// The running state of one list's plan.
struct CopyPlan {
    uint32_t M, nord;
    bool any;
};
// One packet of a list in list order: its status byte.
__host__ __device__ __forceinline__ uint32_t copy_step(CopyPlan &pl, bool bad, uint32_t size, uint32_t put_off,
                                                       uint32_t len, uint32_t code) {
    uint32_t cls = copy_class(bad, size, put_off, len, code);
    if (cls != kCopyCopyable) return cls;
    cls = put_off >= pl.M ? MTCP_GPU_RCVCOPY_FRONT : MTCP_GPU_RCVCOPY_ORDERED;
    pl.nord += cls == MTCP_GPU_RCVCOPY_ORDERED;
    pl.M = copy_umax(pl.M, put_off + len);
    pl.any = true;
    return cls;
}
// The list's end: tcp_ring_buffer.c:304-309 and :317-319 over the whole list.
// Returns whether the window has to move; b holds the new record.
__host__ __device__ __forceinline__ bool copy_finish(const CopyPlan &pl, CopyBuf &b) {
    if (!pl.any) return false;
    const bool trig = (uint64_t)b.head + pl.M >= b.size;          // :304 fired at some packet
    const bool moves = trig && b.head != 0;
    b.last = copy_umax(b.last, pl.M);
    if (trig) b.head = 0;
    b.tail = b.head + b.last;
    return moves;
}

// ---- stores through address-space-1 pointers (global_store, not flat_store) ------
typedef __attribute__((address_space(1))) v4u gsv4u;
typedef __attribute__((address_space(1))) uint32_t gsu32;
typedef __attribute__((address_space(1))) uint16_t gsu16;
typedef __attribute__((address_space(1))) uint8_t gsu8;
typedef __attribute__((address_space(1))) const uint8_t glu8;

// The aligned 16 B piece at byte q of `base` if it holds a byte of [lo, hi),
// else zeros.  LIMITED: a piece that is not wholly below `limit` (the arena's
// last, partial piece) is put together from its bytes below the limit.
template <bool NT, bool LIMITED>
__device__ __forceinline__ v4u copy_piece(uint64_t base, int64_t q, int64_t lo, int64_t hi, uint64_t limit) {
    v4u v = {0u, 0u, 0u, 0u};
    if (!(q + 16 > lo && q < hi)) return v;
    if (LIMITED && (uint64_t)q + 16 > limit) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if ((uint64_t)q + i < limit) w[i >> 2] |= (uint32_t)*reinterpret_cast<glu8 *>(base + q + i) << (8 * (i & 3));
        v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
        return v;
    }
    return NT ? gload_nt(base + (uint64_t)q) : gload(base + (uint64_t)q);
}

// `len` bytes from byte `src` of sbase to byte `dst` of the arena (16 B
// aligned base), by the G lanes sub = 0 .. G - 1.  Every store lies inside
// [dst, dst + len), every load inside the aligned pieces that hold bytes of
// [src, src + len).
template <int G, bool NT, bool LIMITED>
__device__ __forceinline__ void copy_run(uint64_t arena, uint64_t dst, uint64_t sbase, uint64_t src, uint32_t len,
                                         uint32_t sub, uint64_t limit) {
    if (len == 0) return;
    const uint64_t d0 = dst & ~15ull, dend = dst + len;
    const uint32_t nch = (uint32_t)(((dend + 15) >> 4) - (dst >> 4));
    const int64_t slo = (int64_t)src, shi = (int64_t)(src + len);
    const uint32_t sh = (uint32_t)(src - dst) & 15u, k = sh >> 2, b = sh & 3u;
    for (uint32_t c = sub; c < nch; c += G) {
        const uint64_t d = d0 + 16ull * c;
        const int64_t a = slo + ((int64_t)d - (int64_t)dst) - (int64_t)sh;   // the aligned piece that holds d's byte
        const v4u lo = copy_piece<NT, LIMITED>(sbase, a, slo, shi, limit);
        const v4u hi = copy_piece<NT, LIMITED>(sbase, a + 16, slo, shi, limit);
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        uint32_t t[5], o[4];
#pragma unroll
        for (int i = 0; i < 5; ++i) t[i] = k == 0 ? w[i] : k == 1 ? w[i + 1] : k == 2 ? w[i + 2] : w[i + 3];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = __builtin_amdgcn_alignbyte(t[i + 1], t[i], b);
        const uint32_t from = d < dst ? (uint32_t)(dst - d) : 0u, to = d + 16 > dend ? (uint32_t)(dend - d) : 16u;
        if (from == 0 && to == 16) {
            const v4u v = {o[0], o[1], o[2], o[3]};
            *reinterpret_cast<gsv4u *>(arena + d) = v;
            continue;
        }
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t at = 4 * i;
            if (from <= at && at + 4 <= to) {
                *reinterpret_cast<gsu32 *>(arena + d + at) = o[i];
                continue;
            }
#pragma unroll
            for (uint32_t h = 0; h < 2; ++h) {
                const uint32_t ah = at + 2 * h, v = o[i] >> (16 * h);
                if (from <= ah && ah + 2 <= to) {
                    *reinterpret_cast<gsu16 *>(arena + d + ah) = (uint16_t)v;
                    continue;
                }
                if (from <= ah && ah + 1 <= to) *reinterpret_cast<gsu8 *>(arena + d + ah) = (uint8_t)v;
                if (from <= ah + 1 && ah + 2 <= to) *reinterpret_cast<gsu8 *>(arena + d + ah + 1) = (uint8_t)(v >> 8);
            }
        }
    }
}

// ---- prep ---------------------------------------------------------------------
// grid: one lane per position.
__global__ __launch_bounds__(kBlock) void rcvcopy_prep_kernel(const uint8_t *__restrict__ res,
                                                              const uint4 *__restrict__ place,
                                                              const uint2 *__restrict__ desc, uint32_t off_shift,
                                                              uint64_t buf_len, const uint32_t *__restrict__ idx,
                                                              uint32_t n, uint4 *__restrict__ win,
                                                              uint2 *__restrict__ wplan, uint8_t *__restrict__ cstat) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint32_t p = idx[j];
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (p < n) {
        const uint4 pl = place[p];
        const uint32_t w8 = reinterpret_cast<const uint32_t *>(res + 40ull * p)[8];
        const uint2 d = desc[p];
        uint64_t src;
        const uint32_t code = copy_src(pl.w, w8, d.x, d.y & 0xFFFFu, off_shift, buf_len, src);
        if (code) v = make_uint4((uint32_t)src, (uint32_t)(src >> 32), pl.x, (pl.w & 0xFFFFu) | code << 16);
    }
    win[j] = v;
    wplan[j] = make_uint2(0xFFFFFFFFu, 0u);
    cstat[j] = 0;
}

// ---- plan ---------------------------------------------------------------------
// Segment j's list as the copy sees it: [start, stop), stop at seg_stop.
__device__ __forceinline__ void copy_range(uint32_t j, uint32_t n, uint32_t max_id,
                                           const uint32_t *__restrict__ seg_sid,
                                           const uint32_t *__restrict__ seg_start,
                                           const uint32_t *__restrict__ seg_stop, uint32_t &start, uint32_t &stop,
                                           uint32_t &sid) {
    start = min(seg_start[j], n);
    const uint32_t end = max(min(seg_start[j + 1], n), start);
    sid = seg_sid[j];
    stop = sid <= max_id ? min(max(seg_stop[j], start), end) : start;
}
__device__ __forceinline__ uint32_t copy_bcast(uint32_t v, int lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}

// grid: one lane per segment, for n segments (m is known only on the device).
__global__ __launch_bounds__(kBlock) void rcvcopy_plan_kernel(const uint4 *__restrict__ win,
                                                              const uint32_t *__restrict__ idx, uint32_t n,
                                                              uint32_t max_id, const uint32_t *__restrict__ seg_sid,
                                                              const uint32_t *__restrict__ seg_start,
                                                              const uint32_t *__restrict__ nseg,
                                                              const uint32_t *__restrict__ seg_stop, uint4 *rbuf,
                                                              uint64_t arena, uint64_t arena_bytes,
                                                              uint2 *__restrict__ wplan, uint4 *__restrict__ wsum,
                                                              uint8_t *__restrict__ cstat) {
    const uint32_t m = min(nseg[0], n);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t j0 = (blockIdx.x * kBlock + threadIdx.x) - lane;
    if (j0 >= m) return;                                          // the whole wave
    const uint32_t j = j0 + lane;
    const bool valid = j < m;
    uint32_t start = 0, stop = 0, sid = 0xFFFFFFFFu;
    if (valid) copy_range(j, n, max_id, seg_sid, seg_start, seg_stop, start, stop, sid);
    const bool is_stream = valid && sid <= max_id;
    CopyBuf b{};
    bool bad = true;
    if (is_stream) {
        const uint4 r0 = rbuf[2ull * sid], r1 = rbuf[2ull * sid + 1];
        b.data_off = (uint64_t)r0.y << 32 | r0.x, b.size = r0.z, b.head = r0.w;
        b.tail = r1.x, b.last = r1.y, b.r0 = r1.z, b.r1 = r1.w;
        bad = copy_buf_bad(b, arena_bytes);
    }
    CopyPlan pl{0u, 0u, false};
    const bool wide = stop - start > kCopyWaveLen;
    if (!wide)
        for (uint32_t pos = start; pos < stop; ++pos) {
            const uint4 in = win[pos];
            const uint32_t code = in.w >> 16;
            if (code == 0) continue;
            const uint32_t cls = copy_step(pl, bad, b.size, in.z, in.w & 0xFFFFu, code);
            const uint32_t p = idx[pos];
            if (p < n) cstat[p] = (uint8_t)cls;
            wplan[pos] = make_uint2(j, cls);
        }
    // the long lists of these 64 segments, one after the other, as a whole wave
    for (uint64_t todo = __ballot(wide); todo; todo &= todo - 1) {
        const int l = __ffsll((unsigned long long)todo) - 1;
        const uint32_t lstart = copy_bcast(start, l), lstop = copy_bcast(stop, l), lsize = copy_bcast(b.size, l);
        const bool lbad = copy_bcast(bad, l) != 0;
        uint32_t M = 0, nord = 0;
        bool any = false;
        for (uint32_t base = lstart; base < lstop; base += kWave) {
            const uint32_t pos = base + lane;
            uint4 in = make_uint4(0u, 0u, 0u, 0u);
            if (pos < lstop) in = win[pos];
            const uint32_t code = in.w >> 16, len = in.w & 0xFFFFu;
            uint32_t cls = copy_class(lbad, lsize, in.z, len, code);
            const bool can = cls == kCopyCopyable;
            uint32_t incl = can ? in.z + len : 0u;                // the prefix maximum of the ends
#pragma unroll
            for (int d = 1; d < (int)kWave; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d, kWave);
                if ((int)lane >= d) incl = max(incl, up);
            }
            const uint32_t prev = __shfl_up(incl, 1, kWave);
            const uint32_t before = max(M, lane ? prev : 0u);
            if (can) cls = in.z >= before ? MTCP_GPU_RCVCOPY_FRONT : MTCP_GPU_RCVCOPY_ORDERED;
            if (code != 0) {
                const uint32_t p = idx[pos];
                if (p < n) cstat[p] = (uint8_t)cls;
                wplan[pos] = make_uint2(j0 + (uint32_t)l, cls);
            }
            nord += (uint32_t)__popcll(__ballot(can && cls == MTCP_GPU_RCVCOPY_ORDERED));
            any |= __ballot(can) != 0;
            M = max(M, copy_bcast(incl, kWave - 1));
        }
        if ((int)lane == l) pl = CopyPlan{M, nord, any};
    }
    const uint64_t old_at = b.data_off + b.head;
    const uint32_t old_last = b.last;
    const bool moves = copy_finish(pl, b);
    // the windows of the compacting streams, one after the other, as a whole wave
    for (uint64_t todo = __ballot(moves); todo; todo &= todo - 1) {
        const int l = __ffsll((unsigned long long)todo) - 1;
        const uint64_t dst = (uint64_t)copy_bcast((uint32_t)(b.data_off >> 32), l) << 32 | copy_bcast((uint32_t)b.data_off, l);
        const uint64_t src = (uint64_t)copy_bcast((uint32_t)(old_at >> 32), l) << 32 | copy_bcast((uint32_t)old_at, l);
        copy_run<(int)kWave, false, true>(arena, dst, arena, src, copy_bcast(old_last, l), lane, arena_bytes);
    }
    if (pl.any) {
        rbuf[2ull * sid] = make_uint4((uint32_t)b.data_off, (uint32_t)(b.data_off >> 32), b.size, b.head);
        rbuf[2ull * sid + 1] = make_uint4(b.tail, b.last, 0u, 0u);
    }
    if (valid) {
        const uint64_t at = b.data_off + b.head;
        wsum[j] = make_uint4((uint32_t)at, (uint32_t)(at >> 32), pl.nord, moves ? 1u : 0u);
    }
}

// ---- front --------------------------------------------------------------------
// grid: G lanes per position.
template <int G>
__global__ __launch_bounds__(kBlock) void rcvcopy_front_kernel(uint64_t buf, const uint4 *__restrict__ win,
                                                               const uint2 *__restrict__ wplan,
                                                               const uint4 *__restrict__ wsum, uint32_t n,
                                                               uint64_t arena) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t pos = t / G, sub = t % G;
    if (pos >= n) return;
    const uint2 pw = wplan[pos];
    if (pw.y != MTCP_GPU_RCVCOPY_FRONT) return;
    const uint4 in = win[pos], sum = wsum[pw.x];
    const uint64_t dst = ((uint64_t)sum.y << 32 | sum.x) + in.z, src = (uint64_t)in.y << 32 | in.x;
    copy_run<G, true, false>(arena, dst, buf, src, in.w & 0xFFFFu, sub, 0);
}

// ---- ordered ------------------------------------------------------------------
// grid: one lane per segment, for n segments.
__global__ __launch_bounds__(kBlock) void rcvcopy_ordered_kernel(uint64_t buf, const uint4 *__restrict__ win,
                                                                 const uint2 *__restrict__ wplan,
                                                                 const uint4 *__restrict__ wsum, uint32_t n,
                                                                 uint32_t max_id,
                                                                 const uint32_t *__restrict__ seg_sid,
                                                                 const uint32_t *__restrict__ seg_start,
                                                                 const uint32_t *__restrict__ nseg,
                                                                 const uint32_t *__restrict__ seg_stop,
                                                                 uint64_t arena) {
    const uint32_t m = min(nseg[0], n);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t j0 = (blockIdx.x * kBlock + threadIdx.x) - lane;
    if (j0 >= m) return;                                          // the whole wave
    const uint32_t j = j0 + lane;
    uint4 sum = make_uint4(0u, 0u, 0u, 0u);
    uint32_t start = 0, stop = 0, sid = 0;
    if (j < m) {
        sum = wsum[j];
        copy_range(j, n, max_id, seg_sid, seg_start, seg_stop, start, stop, sid);
    }
    for (uint64_t todo = __ballot(sum.z != 0); todo; todo &= todo - 1) {
        const int l = __ffsll((unsigned long long)todo) - 1;
        const uint32_t lstart = copy_bcast(start, l), lstop = copy_bcast(stop, l);
        const uint64_t at = (uint64_t)copy_bcast(sum.y, l) << 32 | copy_bcast(sum.x, l);
        for (uint32_t base = lstart; base < lstop; base += kWave) {
            const uint32_t pos = base + lane;
            uint4 in = make_uint4(0u, 0u, 0u, 0u);
            bool mine = false;
            if (pos < lstop) {
                const uint2 pw = wplan[pos];
                mine = pw.x == j0 + (uint32_t)l && pw.y == MTCP_GPU_RCVCOPY_ORDERED;
                if (mine) in = win[pos];
            }
            for (uint64_t pk = __ballot(mine); pk; pk &= pk - 1) {
                const int k = __ffsll((unsigned long long)pk) - 1;
                const uint64_t src = (uint64_t)copy_bcast(in.y, k) << 32 | copy_bcast(in.x, k);
                copy_run<(int)kWave, true, false>(arena, at + copy_bcast(in.z, k), buf, src, copy_bcast(in.w, k) & 0xFFFFu,
                                                  lane, 0);
                __threadfence();                                  // this packet's stores are complete before the next one's begin
            }
        }
    }
}
}  // namespace mg
