// flowtab_kernels.hpp — gfx950 kernels of the device flow table (SURVEY §8
// row f9): a mirror in HBM of mTCP's tcp_flow_table (mtcp/src/fhash.c:16-121),
// so that the rx batch's last read-only step, StreamHTSearch
// (mtcp/src/tcp_in.c:1181-1186, fhash.c:103-121), runs behind the rx launch.
//
// The reference's table is 131 072 TAILQ bins of stream pointers.  The mirror
// is one array of cap 16 B slots, open addressing with linear probing:
//
//   slot   {saddr, daddr, sport | dport << 16, id}: the 12 key bytes HashFlow
//          reads (tcp_stream.c:56-90), in the stream's orientation, and the
//          caller's stream number.  id 0xFFFFFFFF: never used (EMPTY);
//          0xFFFFFFFE: removed (TOMB, key words stale).
//   home   hash_flow32(key) & (cap - 1): the unmasked Jenkins value of
//          HashFlow, so the pinned 17-bit bin is the home's low bits (all of
//          it for cap >= 2^17).
//
// A lookup's answer is the lowest id among the live slots with the record's
// key (include/mtcp_gpu_flowtab.h has the contract), so slot order carries no
// meaning: an insert takes the first EMPTY or TOMB slot from home, a remove
// leaves a TOMB, and every live entry of a key lies between its home and the
// first EMPTY slot behind it, which is where lookups and removes stop.
//
// No lane waits for another.  Every probe loop runs at most cap steps.  A
// slot is claimed or released by one agent-scope compare-and-swap on its id
// word (L2 is not coherent across XCDs; the atomic goes to the coherent
// point); a lane that loses the swap goes on to the next slot and never tries
// the same one again.  The key words are written with plain stores after the
// claim: inserts look at id words only, and removes and lookups run in other
// launches, ordered behind this one by the stream.  Counters move once per
// wave (one ballot, one atomic add by lane 0), not once per lane.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu.h"
#include "../../include/mtcp_gpu_flowtab.h"
#include "rx_kernels.hpp"

namespace mg {

constexpr uint32_t kFlowEmpty = 0xFFFFFFFFu;
constexpr uint32_t kFlowTomb = 0xFFFFFFFEu;
static_assert(MTCP_GPU_FLOW_NONE == kFlowEmpty && MTCP_GPU_FLOW_MISS == kFlowTomb &&
              MTCP_GPU_FLOWTAB_MAX_ID < kFlowTomb, "a lookup's minimum over ids relies on this order");

// counters of the 16 B stats block (mtcp_gpu_flowtab_counters)
enum { kFtLive = 0, kFtTombs = 1, kFtInsertFailed = 2, kFtRemoveMissed = 3 };

__host__ __device__ __forceinline__ uint32_t flowtab_home(const uint32_t (&key)[3], uint32_t mask) {
    return hash_flow32(key) & mask;
}

__device__ __forceinline__ uint32_t *slot_id(uint4 *slots, uint32_t s) {
    return reinterpret_cast<uint32_t *>(slots + s) + 3;
}

// ctr += by * (lanes of this wave with flag); every lane of the wave calls it.
__device__ __forceinline__ void wave_count(uint32_t *ctr, bool flag, uint32_t by = 1u) {
    const uint64_t m = __ballot(flag);
    if (m && (threadIdx.x & (kWave - 1)) == 0)
        (void)__hip_atomic_fetch_add(ctr, by * (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Puts e into the first EMPTY or TOMB slot from its home.  Returns 0 (table
// full after cap probes), 1 (took an EMPTY slot) or 2 (took a TOMB).
__device__ __forceinline__ uint32_t flowtab_place(uint4 *slots, uint32_t mask, uint4 e) {
    const uint32_t key[3] = {e.x, e.y, e.z};
    const uint32_t home = flowtab_home(key, mask);
    for (uint32_t p = 0; p <= mask; ++p) {
        const uint32_t s = (home + p) & mask;
        uint32_t *idw = slot_id(slots, s);
        const uint32_t cur = __hip_atomic_load(idw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur < kFlowTomb) continue;                              // live
        uint32_t expect = cur;
        if (__hip_atomic_compare_exchange_strong(idw, &expect, e.w, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT)) {
            uint32_t *w = reinterpret_cast<uint32_t *>(slots + s);
            *reinterpret_cast<uint2 *>(w) = make_uint2(e.x, e.y);
            w[2] = e.z;
            return cur == kFlowTomb ? 2u : 1u;
        }                                                           // lost: the slot is another lane's now
    }
    return 0u;
}

// StreamHTRemove (fhash.c:89-101), one lane per entry: the first slot from
// home with the entry's key AND id becomes a TOMB.
__global__ __launch_bounds__(kBlock) void flowtab_remove_kernel(uint4 *__restrict__ slots, uint32_t mask,
                                                                const uint4 *__restrict__ del, uint32_t n,
                                                                uint32_t *__restrict__ stats) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += stride) {   // uniform per workgroup
        const uint32_t i = base + threadIdx.x;
        bool removed = false;
        if (i < n) {
            const uint4 e = del[i];
            if (e.w <= MTCP_GPU_FLOWTAB_MAX_ID) {
                const uint32_t key[3] = {e.x, e.y, e.z};
                const uint32_t home = flowtab_home(key, mask);
                for (uint32_t p = 0; p <= mask; ++p) {
                    const uint32_t s = (home + p) & mask;
                    const uint4 v = slots[s];
                    if (v.w == kFlowEmpty) break;
                    if (v.w != e.w || v.x != e.x || v.y != e.y || v.z != e.z) continue;
                    uint32_t expect = e.w;
                    if (__hip_atomic_compare_exchange_strong(slot_id(slots, s), &expect, kFlowTomb, __ATOMIC_RELAXED,
                                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                        removed = true;
                        break;
                    }                                               // lost to a lane removing the same pair
                }
            }
        }
        wave_count(stats + kFtLive, removed, 0xFFFFFFFFu);          // - 1 each
        wave_count(stats + kFtTombs, removed);
        wave_count(stats + kFtRemoveMissed, i < n && !removed);
    }
}

// StreamHTInsert (fhash.c:68-87), one lane per entry.
__global__ __launch_bounds__(kBlock) void flowtab_insert_kernel(uint4 *__restrict__ slots, uint32_t mask,
                                                                const uint4 *__restrict__ ins, uint32_t n,
                                                                uint32_t *__restrict__ stats) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += stride) {
        const uint32_t i = base + threadIdx.x;
        uint32_t how = 0;
        if (i < n) {
            const uint4 e = ins[i];
            if (e.w <= MTCP_GPU_FLOWTAB_MAX_ID) how = flowtab_place(slots, mask, e);
        }
        wave_count(stats + kFtLive, how != 0);
        wave_count(stats + kFtTombs, how == 2, 0xFFFFFFFFu);
        wave_count(stats + kFtInsertFailed, i < n && how == 0);
    }
}

// Rehash: every live slot of the old array into the fresh one (all EMPTY,
// same cap, so a place cannot fail; counted all the same).  live is counted
// anew (the host zeroed live and tombs on the stream before this launch).
__global__ __launch_bounds__(kBlock) void flowtab_rehash_kernel(const uint4 *__restrict__ old_slots,
                                                                uint4 *__restrict__ slots, uint32_t mask,
                                                                uint32_t *__restrict__ stats) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t base = blockIdx.x * kBlock; base <= mask; base += stride) {
        const uint32_t i = base + threadIdx.x;
        uint32_t how = 0;
        bool live = false;
        if (i <= mask) {
            const uint4 e = old_slots[i];
            live = e.w <= MTCP_GPU_FLOWTAB_MAX_ID;
            if (live) how = flowtab_place(slots, mask, e);
        }
        wave_count(stats + kFtLive, how != 0);
        wave_count(stats + kFtInsertFailed, live && how == 0);
    }
}

// StreamHTSearch (fhash.c:103-121) for every record of an rx batch, one lane
// per 40 B record: saddr @0, daddr @4, sport|dport @8, verdict @36, loaded as
// flow_hash_kernel loads them.  G slots are loaded per probe step (all G loads
// issued before the first compare).
template <int G>
__global__ __launch_bounds__(kBlock) void flowtab_lookup_kernel(const mtcp_gpu_result *__restrict__ res,
                                                                uint32_t n, const uint4 *__restrict__ slots,
                                                                uint32_t mask, uint32_t *__restrict__ sid,
                                                                uint32_t *__restrict__ bins) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const uint32_t *r = reinterpret_cast<const uint32_t *>(res + i);
        const uint32_t saddr = r[0], daddr = r[1], ports = r[2], verdict = r[9] & 0xFFu;
        uint32_t key[3];
        flow_key(saddr, daddr, ports, key);                         // rx_kernels.hpp, as flow_bin
        const uint32_t h = hash_flow32(key);
        const bool ok = verdict == MTCP_GPU_V_TCP_OK;
        uint32_t best = MTCP_GPU_FLOW_NONE;
        if (ok) {
            best = MTCP_GPU_FLOW_MISS;
            const uint32_t home = h & mask;
            bool end = false;
            for (uint32_t p = 0; p <= mask && !end; p += G) {       // cap is a multiple of G
                uint4 v[G];
#pragma unroll
                for (int k = 0; k < G; ++k) v[k] = slots[(home + p + k) & mask];
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    if (end) continue;
                    if (v[k].w == kFlowEmpty) {
                        end = true;
                    } else if (v[k].x == key[0] && v[k].y == key[1] && v[k].z == key[2]) {
                        best = min(best, v[k].w);                   // a TOMB's id is FLOW_MISS itself
                    }
                }
            }
        }
        sid[i] = best;
        if (bins) bins[i] = ok ? h & (MTCP_GPU_NUM_BINS_FLOWS - 1) : MTCP_GPU_FLOW_NONE;
    }
}

}  // namespace mg
