// mtcp_gpu.hip — the C ABI of include/mtcp_gpu.h: contexts, launches and the
// host-memory pipelines around the gfx950 kernels of rx_kernels.hpp.
//
// Product code only: there is no CPU fallback here.  When no GPU is usable
// every entry point returns an error code, and the caller (mTCP) keeps its
// software path exactly as dev_ioctl returning -1 would make it
// (mtcp/src/ip_in.c:29-31, tcp_in.c:1160-1164).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/mtcp_gpu.h"
#include "../../include/mtcp_gpu_flowtab.h"
#include "../../include/mtcp_gpu_group.h"
#include "../../include/mtcp_gpu_rcvwalk.h"
#include "../../include/mtcp_gpu_ackwalk.h"
#include "../../include/mtcp_gpu_ackgen.h"
#include "../../include/mtcp_gpu_datagen.h"
#include "../../include/mtcp_gpu_rcvread.h"
#include "../../include/mtcp_gpu_rtosweep.h"
#include "../../include/mtcp_gpu_sndwrite.h"
#include "../../include/mtcp_gpu_rcvcopy.h"
#include "../../include/mtcp_gpu_steer.h"
#include "../../include/mtcp_gpu_tcpopt.h"
#include "../../include/mtcp_gpu_txbuild.h"
#include "../../include/mtcp_gpu_txseg.h"
#include "ctx_internal.hpp"
#include "dispatch.hpp"
#include "flow_kernels.hpp"
#include "flowtab_kernels.hpp"
#include "group_kernels.hpp"
#include "host_call.hpp"
#include "host_copy.hpp"
#include "stage_layout.hpp"
#include "park.hpp"
#include "rcvwalk_kernels.hpp"
#include "ackwalk_kernels.hpp"
#include "ackgen_kernels.hpp"
#include "datagen_kernels.hpp"
#include "rtosweep_kernels.hpp"
#include "rcvread_kernels.hpp"
#include "sndwrite_kernels.hpp"   // last: the kernels of the rows before it keep their place in the code object
#include "rcvcopy_kernels.hpp"
#include "rx_kernels.hpp"
#include "rx_span.hpp"
#include "steer_kernels.hpp"
#include "tcpopt_kernels.hpp"
#include "txbuild_kernels.hpp"
#include "txseg_kernels.hpp"
#include "wait.hpp"

namespace {

using namespace mtcp_host;   // Stage, HostCall and the staging constants (host_call.hpp)
using mtcp_wait::Deadline;
using mtcp_wait::drain;

}  // namespace

struct mtcp_gpu_ctx {
    int device = 0;
    int num_cu = 256;
    uint32_t flags = 0;
    uint32_t rss_nq = 1;
    uint32_t rss_endian = 0;
    uint32_t rss_key_w[4] = {0, 0, 0, 0};        // key bytes 0..15, big-endian words
    int sched = 0;                               // Sched: kSchedAuto unless MTCP_GPU_SCHED forces one
    hipStream_t stream = nullptr;
    const uint32_t *d_rss_tables = nullptr;      // shared, immutable (rss_tables_for)
    uint32_t wait_us = 0;                        // mtcp_gpu_set_wait_limit (0: no limit)
    Stage stage[kStages];
    uint8_t *h_gather = nullptr;                 // pinned, for rx_ptrs
    uint64_t h_gather_cap = 0;
    mtcp_gpu_desc *h_gather_desc = nullptr;
    uint32_t h_gather_desc_cap = 0;
    const char *last_kernel = "";                // mtcp_gpu_last_kernel
    // a host call's bounded wait gave up: work of that call may still read
    // or write the staging, so nothing is issued, staged or freed on this
    // context again (every call answers EIO)
    bool abandoned = false;
};

namespace {

// util/rss.c:13-105 (BuildKeyCache), then the 24 nibble tables the kernel
// XORs: table[t][v] = XOR of cache[4t + m] over the bits of nibble v, MSB
// first (nibble t of the 96-bit input sip|dip|sp|dp, most significant first).
void build_rss_tables(const uint8_t key[40], uint32_t *tables) {
    uint32_t cache[96];
    uint32_t result = ((uint32_t)key[0] << 24) | ((uint32_t)key[1] << 16) |
                      ((uint32_t)key[2] << 8) | (uint32_t)key[3];
    uint32_t idx = 32;
    for (int i = 0; i < 96; i++, idx++) {
        cache[i] = result;
        const uint32_t bit = ((key[idx / 8] << (idx % 8)) & 0x80) ? 1u : 0u;
        result = (result << 1) | bit;
    }
    for (int t = 0; t < 24; ++t)
        for (int v = 0; v < 16; ++v) {
            uint32_t h = 0;
            for (int m = 0; m < 4; ++m)
                if (v & (0x8 >> m)) h ^= cache[4 * t + m];
            tables[t * 16 + v] = h;
        }
}

// Two 256-thread workgroups per CU (8 waves): measured fastest on MI355X for
// this streaming kernel (fewer concurrent streams keep HBM efficiency up;
// tools/rx_variants.hip sweeps 1..4 per CU).  Each wave walks its passes.
uint32_t grid_for(const mtcp_gpu_ctx *ctx, uint32_t n) {
    const uint32_t groups = (n + mg::kWave - 1) / mg::kWave;
    const uint32_t blocks = (groups + mg::kWavesPerBlock - 1) / mg::kWavesPerBlock;
    const uint32_t cap = (uint32_t)ctx->num_cu * 2;
    return std::max(1u, std::min(blocks, cap));
}

// Two workgroups share each CU, and the first one dispatched wins the memory
// arbitration: per-wave s_memrealtime stamps of C2 (tools/rx_variants
// stampsab) show the second workgroup ending ~7 us after the first, with
// the CU half-occupied meanwhile.  The second workgroup runs at s_setprio(1)
// for its first four passes (rx_kernel PRIO 5), which evens the two (C2:
// 242.9-245.8 -> 239.7-240.8 us in the same process); the other schedules
// showed no change and keep the default.
template <int SCHED, bool LALIGN>
constexpr int prio_for() { return SCHED == mg::kSchedUnrolled && !LALIGN ? 5 : 0; }

template <int MODE, bool RSS, int SCHED, bool LALIGN, bool CMP>
void launch_one(dim3 grid, dim3 block, hipStream_t st, const mg::KParams &kp) {
    // tx fill streams its frames through L2 normally (NT off): its check-field
    // writes at the end then find part of the last passes' lines resident
    // (f1: 324 -> 317 us on 1 M x 1500 B; rx keeps the non-temporal stream)
    constexpr bool kNT = MODE != mg::kTxChunk;
    // multi-trip frames in the unrolled schedule: odd rows walk their trips
    // backwards so neighbouring frames' shared lines are read in one step
    // (C5: 4.768 -> 4.737 GB per launch = chunk + descriptors, no line twice)
    constexpr bool kRev = LALIGN && SCHED == mg::kSchedUnrolled;
    // runs of 16 packets for the size-sorted chunk schedule (C3-shaped
    // batches): its per-lane descriptors come in 128 B pieces instead of 64 B
    // (tools/rx_variants c3: 133.8 vs 134.9 us, records identical); the
    // unrolled schedule keeps 8 and loads them per workgroup (rx_kernel COOP)
    constexpr int kB = SCHED == mg::kSchedSorted && !LALIGN && MODE == mg::kRxChunk ? 16 : 8;
    hipLaunchKernelGGL((mg::rx_kernel<MODE, RSS, SCHED, LALIGN, 0, 8, kB, kNT, 6, kRev, false,
                                      prio_for<SCHED, LALIGN>(), mg::kWavesPerBlock, 0, CMP>),
                       grid, block, 0, st, kp);
}

template <int MODE, bool RSS, bool CMP>
const char *launch_sched(dim3 grid, dim3 block, hipStream_t st, const mg::KParams &kp, uint64_t slot,
                         uint32_t batch_n) {
    // the schedule (dispatch.hpp big_schedule) is chosen once per batch
    // (batch_n: the whole batch, not this launch's share of it)
    const int b = big_schedule(MODE == mg::kRxPtrs, slot, batch_n);
    if constexpr (MODE == mg::kRxPtrs) {
        launch_one<MODE, RSS, mg::kSchedSorted, true, CMP>(grid, block, st, kp);
    } else if (b == kBigSorted) {
        launch_one<MODE, RSS, mg::kSchedSorted, false, CMP>(grid, block, st, kp);
    } else if (b == kBigUnrolledLineAligned) {
        launch_one<MODE, RSS, mg::kSchedUnrolled, true, CMP>(grid, block, st, kp);
    } else {
        launch_one<MODE, RSS, mg::kSchedUnrolled, false, CMP>(grid, block, st, kp);
    }
    return kernel_name(kSchedBig, b, slot);
}

// A wave holds its results for up to kHeldPasses passes and stores them in
// one burst at the end (rx_kernel DEFER); a batch needing more passes would
// flush mid-stream, which costs more than a second launch (C4's 2 M x 1500 B
// per GPU: one launch 511 us, two launches of 1 M ~486 us).  So a batch is
// cut into launches of at most grid x 4 waves x 64 x kHeldPasses packets.
constexpr uint32_t kHeldPasses = 8;

// The kernel choice (batch size, average slot, size hint) is dispatch.hpp's
// pick_sched / big_schedule, shared with the CPU test of its rules.

template <int MODE, bool RSS>
const char *launch_small(int sched, uint32_t n, uint64_t slot, hipStream_t st, const mg::KParams &kp) {
    if (sched == kSchedWave) {
        const dim3 grid((n + mg::kWavesPerBlock - 1) / mg::kWavesPerBlock);
        if (slot <= kWaveShortUpToSlot) {
            hipLaunchKernelGGL((mg::rx_wave_kernel<MODE, RSS, 0, 1, 2>), grid, dim3(mg::kBlock), 0, st, kp);
            return "rx_wave_kernel<2 loads>";
        }
        hipLaunchKernelGGL((mg::rx_wave_kernel<MODE, RSS>), grid, dim3(mg::kBlock), 0, st, kp);
        return "rx_wave_kernel<10 loads>";
    } else if (sched == kSchedQuad) {
        constexpr int kBlk = mg::kQuadBlock;
        constexpr uint32_t P = mg::GroupShape<4, kBlk>::P;
        hipLaunchKernelGGL((mg::rx_group_kernel<MODE, RSS, 4, 0, 1, kBlk>), dim3((n + P - 1) / P), dim3(kBlk), 0,
                           st, kp);
        return "rx_group_kernel<quad>";
    } else if (sched == kSchedOct) {
        constexpr int kBlk = mg::kOctBlock;
        constexpr uint32_t P = mg::GroupShape<8, kBlk>::P;
        hipLaunchKernelGGL((mg::rx_group_kernel<MODE, RSS, 8, 0, 1, kBlk>), dim3((n + P - 1) / P), dim3(kBlk), 0,
                           st, kp);
        return "rx_group_kernel<oct>";
    } else if (sched == kSchedSpan) {
        if constexpr (!mg::is_tx(MODE)) {
            hipLaunchKernelGGL((mg::rx_span_kernel<MODE, RSS>), dim3((n + mg::kSpanP - 1) / mg::kSpanP),
                               dim3(mg::kSpanBlock), 0, st, kp);
            return "rx_span_kernel";
        }
    }
    constexpr uint32_t P = mg::GroupShape<16>::P;
    hipLaunchKernelGGL((mg::rx_group_kernel<MODE, RSS, 16>), dim3((n + P - 1) / P), dim3(mg::kGroupBlock), 0,
                       st, kp);
    return "rx_group_kernel<row>";
}

// bytes per rx record: 40 (mtcp_gpu_result) or 16 (mtcp_gpu_result16)
uint64_t record_size(const mg::KParams &kp) { return kp.compact ? 16 : 40; }
uint64_t record_size(const mtcp_gpu_ctx *ctx) { return (ctx->flags & MTCP_GPU_F_COMPACT) ? 16 : 40; }

template <int MODE>
int launch(mtcp_gpu_ctx *ctx, const mg::KParams &kp, hipStream_t st, const mtcp_gpu_size_hint *hint = nullptr) {
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (kp.n == 0) return MTCP_GPU_OK;
    const bool rss = !mg::is_tx(MODE) && (ctx->flags & MTCP_GPU_F_RSS);
    const bool ptrs = MODE == mg::kRxPtrs || MODE == mg::kTxPtrs;
    const uint64_t avg_slot = ptrs ? 1024 : kp.buf_len / kp.n;
    const int sched = pick_sched(ctx->sched, kp.n, avg_slot, MODE == mg::kTxPtrs || kp.tx_report != nullptr,
                                 !mg::is_tx(MODE), !ptrs && narrow_batch(hint));
    if (sched != kSchedBig) {
        ctx->last_kernel = rss ? launch_small<MODE, true>(sched, kp.n, avg_slot, st, kp)
                               : launch_small<MODE, false>(sched, kp.n, avg_slot, st, kp);
        return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
    }
    if constexpr (MODE != mg::kTxPtrs) {
    const dim3 grid(grid_for(ctx, kp.n)), block(mg::kBlock);
    const uint64_t slot = kp.n ? kp.buf_len / kp.n : 0;       // the whole batch's average slot
    const uint32_t cap = grid.x * mg::kWavesPerBlock * mg::kWave * kHeldPasses;
    for (uint32_t first = 0; first < kp.n; first += cap) {
        mg::KParams sub = kp;
        sub.n = std::min(kp.n - first, cap);
        if (MODE == mg::kRxPtrs) {
            sub.ptrs = kp.ptrs + first;
            sub.lens = kp.lens + first;
        } else {
            sub.desc = kp.desc + first;
        }
        if (MODE != mg::kTxChunk)
            sub.out = reinterpret_cast<mtcp_gpu_result *>(reinterpret_cast<uint8_t *>(kp.out) +
                                                          (uint64_t)first * record_size(kp));
        if (kp.bins) sub.bins = kp.bins + first;
        if constexpr (mg::is_tx(MODE)) {
            ctx->last_kernel = launch_sched<MODE, false, false>(grid, block, st, sub, slot, kp.n);
        } else if (kp.compact) {
            ctx->last_kernel = rss ? launch_sched<MODE, true, true>(grid, block, st, sub, slot, kp.n)
                                   : launch_sched<MODE, false, true>(grid, block, st, sub, slot, kp.n);
        } else {
            ctx->last_kernel = rss ? launch_sched<MODE, true, false>(grid, block, st, sub, slot, kp.n)
                                   : launch_sched<MODE, false, false>(grid, block, st, sub, slot, kp.n);
        }
    }
    }
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

mg::KParams base_params(mtcp_gpu_ctx *ctx) {
    mg::KParams kp{};
    kp.rss_tables = ctx->d_rss_tables;
    kp.rss_nq = ctx->rss_nq;
    kp.rss_endian = ctx->rss_endian;
    for (int i = 0; i < 4; ++i) kp.rss_key[i] = ctx->rss_key_w[i];
    kp.compact = (ctx->flags & MTCP_GPU_F_COMPACT) ? 1u : 0u;
    return kp;
}

// results of the device entry points: 8 B aligned (40 B records, stored in
// 8 and 16 B pieces), 16 B aligned for the compact records (one 16 B store)
uintptr_t out_align(const mtcp_gpu_ctx *ctx) { return (ctx->flags & MTCP_GPU_F_COMPACT) ? 15 : 7; }

hipStream_t pick(mtcp_gpu_ctx *ctx, void *stream) {
    return stream ? reinterpret_cast<hipStream_t>(stream) : ctx->stream;
}

// a stage's buffers back to park.hpp (its stream has no work on them);
// may_free = false inside a bounded call: nothing may wait on the device
void stage_release_buf(Stage &s, bool may_free) {
    mtcp_park::release(s.d_buf, s.buf_cap, mtcp_park::kDevice, may_free);
    s.d_buf = nullptr;
    s.buf_cap = 0;
}
void stage_release_pkts(Stage &s, bool may_free) {
    mtcp_park::release(s.d_desc, (size_t)s.pkt_cap * sizeof(mtcp_gpu_desc), mtcp_park::kDevice, may_free);
    mtcp_park::release(s.d_out, (size_t)s.pkt_cap * sizeof(mtcp_gpu_result), mtcp_park::kDevice, may_free);
    s.d_desc = nullptr;
    s.d_out = nullptr;
    s.pkt_cap = 0;
}
constexpr size_t kStageOptBytes = (size_t)kStagePkts * sizeof(mtcp_gpu_tcpopt);
void stage_release_opts(Stage &s, bool may_free) {
    mtcp_park::release(s.d_opt, kStageOptBytes, mtcp_park::kDevice, may_free);
    mtcp_park::release(s.h_opt, kStageOptBytes, mtcp_park::kHost, may_free);
    s.d_opt = s.h_opt = nullptr;
}
void stage_release_host(Stage &s, bool may_free) {
    mtcp_park::release(s.h_in, s.h_in_cap, mtcp_park::kHost, may_free);
    mtcp_park::release(s.h_out, s.h_out_cap, mtcp_park::kHost, may_free);
    s.h_in = s.h_out = nullptr;
    s.h_in_cap = s.h_out_cap = 0;
}

// A wait of a host call ended: past the deadline the context is abandoned
// (the work it gave up on may still use the staging), and the call answers
// MTCP_GPU_ETIMEDOUT.
int waited(mtcp_gpu_ctx *ctx, int rc) {
    if (rc == MTCP_GPU_ETIMEDOUT) ctx->abandoned = true;
    return rc;
}

// The stage's stream: stage 0 is the context's own; the others are created
// on the first call that spans more than one stage.
int stage_stream(mtcp_gpu_ctx *ctx, Stage &s) {
    if (s.stream) return MTCP_GPU_OK;
    if (&s == &ctx->stage[0]) {
        s.stream = ctx->stream;
        return MTCP_GPU_OK;
    }
    if (!HIP_OK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking))) return MTCP_GPU_EIO;
    s.own_stream = true;
    return MTCP_GPU_OK;
}

int stage_reserve(mtcp_gpu_ctx *ctx, Stage &s, uint64_t bytes, uint32_t pkts, const Deadline &dl) {
    if (ctx->abandoned) return MTCP_GPU_EIO;
    int rc = stage_stream(ctx, s);
    if (rc != MTCP_GPU_OK) return rc;
    // growing releases buffers that the stage's previous batch may still
    // use: drain that batch first (park.hpp releases without any device wait)
    if ((bytes > s.buf_cap || pkts > s.pkt_cap) && (rc = waited(ctx, drain(s.stream, dl))) != MTCP_GPU_OK)
        return rc;
    if (bytes > s.buf_cap) {
        stage_release_buf(s, !dl.bounded);
        const uint64_t cap = (bytes + 4095) & ~4095ull;
        if (!HIP_OK(mtcp_park::alloc(&s.d_buf, cap, mtcp_park::kDevice))) return MTCP_GPU_ENOMEM;
        s.buf_cap = cap;
    }
    if (pkts > s.pkt_cap) {
        stage_release_pkts(s, !dl.bounded);
        if (!HIP_OK(mtcp_park::alloc(&s.d_desc, (size_t)pkts * sizeof(mtcp_gpu_desc), mtcp_park::kDevice)))
            return MTCP_GPU_ENOMEM;
        if (!HIP_OK(mtcp_park::alloc(&s.d_out, (size_t)pkts * sizeof(mtcp_gpu_result), mtcp_park::kDevice))) {
            mtcp_park::release(s.d_desc, (size_t)pkts * sizeof(mtcp_gpu_desc), mtcp_park::kDevice, !dl.bounded);
            s.d_desc = nullptr;
            return MTCP_GPU_ENOMEM;
        }
        s.pkt_cap = pkts;
    }
    return MTCP_GPU_OK;
}

// Pinned host buffers of a stage: in_bytes of bounce for the caller's input
// (a bounded call copies it there first), out_bytes for what comes back.
// The stage's stream has no work on them (a grown buffer is released).
int stage_host(mtcp_gpu_ctx *ctx, Stage &s, uint64_t in_bytes, uint64_t out_bytes, const Deadline &dl) {
    int rc = MTCP_GPU_OK;
    if ((in_bytes > s.h_in_cap || out_bytes > s.h_out_cap) && s.stream &&
        (rc = waited(ctx, drain(s.stream, dl))) != MTCP_GPU_OK)
        return rc;
    if (in_bytes > s.h_in_cap) {
        mtcp_park::release(s.h_in, s.h_in_cap, mtcp_park::kHost, !dl.bounded);
        s.h_in = nullptr;
        s.h_in_cap = 0;
        const uint64_t cap = (in_bytes + 4095) & ~4095ull;
        if (!HIP_OK(mtcp_park::alloc(&s.h_in, cap, mtcp_park::kHost))) return MTCP_GPU_ENOMEM;
        s.h_in_cap = cap;
    }
    if (out_bytes > s.h_out_cap) {
        mtcp_park::release(s.h_out, s.h_out_cap, mtcp_park::kHost, !dl.bounded);
        s.h_out = nullptr;
        s.h_out_cap = 0;
        const uint64_t cap = (out_bytes + 4095) & ~4095ull;
        if (!HIP_OK(mtcp_park::alloc(&s.h_out, cap, mtcp_park::kHost))) return MTCP_GPU_ENOMEM;
        s.h_out_cap = cap;
    }
    return MTCP_GPU_OK;
}

// The end of a host call that used stages [0, nstages): every stage's
// stream drained within the call's deadline, then what a bounded call's
// batches still owe the caller copied out (only if the result is MTCP_GPU_OK).
// Returns rc if every drain succeeded, MTCP_GPU_ETIMEDOUT (the context
// abandoned) past the deadline — or at once, without a further wait, if a
// wait of the call gave up before.
int finish_call(mtcp_gpu_ctx *ctx, int rc, const Deadline &dl, int nstages) {
    for (int i = 0; i < nstages && rc != MTCP_GPU_ETIMEDOUT; ++i) {
        Stage &s = ctx->stage[i];
        if (!s.stream) continue;
        const int r = waited(ctx, drain(s.stream, dl));
        if (r == MTCP_GPU_ETIMEDOUT || rc == MTCP_GPU_OK) rc = r;
    }
    for (auto &s : ctx->stage) rc == MTCP_GPU_OK ? stage_copy_out(s) : stage_drop(s);
    return rc;
}

// A bounded call reuses stage s for its next batch: the batch it holds
// finishes (within the deadline) and its records are copied out.
int stage_collect(mtcp_gpu_ctx *ctx, Stage &s, const Deadline &dl) {
    if (!s.npend) return MTCP_GPU_OK;
    const int rc = waited(ctx, drain(s.stream, dl));
    if (rc == MTCP_GPU_OK) stage_copy_out(s);
    return rc;
}

// host_call.hpp's backend: the copies of a call on stage 0 go on the
// context's stream, and a round ends in finish_call.
struct HipBackend {
    mtcp_gpu_ctx *ctx;
    const Deadline &dl;
    bool copy(void *dst, const void *src, uint64_t bytes, bool up) {
        return HIP_OK(hipMemcpyAsync(dst, src, bytes, up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost,
                                     ctx->stage[0].stream));
    }
    int drain(int rc) { return finish_call(ctx, rc, dl, 1); }
};
using Call = HostCall<HipBackend>;

// The option records' staging of a stage (mtcp_gpu_rx_chunk_opts): allocated
// once, at full stage size, so it never grows under a batch in flight.
int stage_opts(Stage &s, bool bounce) {
    if (!s.d_opt && !HIP_OK(mtcp_park::alloc(&s.d_opt, kStageOptBytes, mtcp_park::kDevice)))
        return MTCP_GPU_ENOMEM;
    if (bounce && !s.h_opt && !HIP_OK(mtcp_park::alloc(&s.h_opt, kStageOptBytes, mtcp_park::kHost)))
        return MTCP_GPU_ENOMEM;
    return MTCP_GPU_OK;
}

// The option kernel (tcpopt_kernels.hpp) over the frames of kp, reading the
// rx records at `res` (this context's record form); one lane per packet, up
// to 8 workgroups per CU, grid-stride beyond.
template <bool PTRS>
int launch_tcpopt(mtcp_gpu_ctx *ctx, const mg::KParams &kp, const void *res, mtcp_gpu_tcpopt *opt,
                  hipStream_t st) {
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (kp.n == 0) return MTCP_GPU_OK;
    mg::OptParams op{};
    op.buf = kp.buf;
    op.buf_len = kp.buf_len;
    op.base_sub = kp.base_sub;
    op.desc = kp.desc;
    op.ptrs = kp.ptrs;
    op.lens = kp.lens;
    op.n = kp.n;
    op.off_shift = kp.off_shift;
    op.res = res;
    op.opt = reinterpret_cast<uint4 *>(opt);
    const dim3 grid(std::min<uint32_t>((kp.n + mg::kBlock - 1) / mg::kBlock, (uint32_t)ctx->num_cu * 8));
    if (kp.compact)
        hipLaunchKernelGGL((mg::tcpopt_kernel<PTRS, true>), grid, dim3(mg::kBlock), 0, st, op);
    else
        hipLaunchKernelGGL((mg::tcpopt_kernel<PTRS, false>), grid, dim3(mg::kBlock), 0, st, op);
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

// The Toeplitz tables of one RSS key on one device (build_rss_tables):
// built and uploaded by the first context opened with that key, then shared
// by every later one, never written again and never freed.  So a kernel
// still reading them — a *_dev launch on a caller's stream that has not
// finished when its context is closed — reads the key it was launched with,
// whatever contexts open or close meanwhile.  At most one set of 1.5 KiB
// per distinct key and device.
struct RssTables {
    int device;
    uint8_t key[40];
    uint32_t host[mg::kRssTableWords];           // the upload's source, kept with the tables
    uint32_t *d;
};

std::mutex &rss_mutex() {
    static std::mutex *m = new std::mutex;
    return *m;
}
std::vector<RssTables *> &rss_cache() {
    static std::vector<RssTables *> *v = new std::vector<RssTables *>;
    return *v;
}

// Bound of the one wait at mtcp_gpu_open (a new key's table upload on the
// new context's stream), before any limit can be set on the context.
constexpr uint32_t kOpenWaitUs = 2000000;

int rss_tables_for(int device, const uint8_t key[40], hipStream_t st, const uint32_t **out) {
    {
        std::lock_guard<std::mutex> lk(rss_mutex());
        for (const RssTables *t : rss_cache())
            if (t->device == device && memcmp(t->key, key, 40) == 0) {
                *out = t->d;
                return MTCP_GPU_OK;
            }
    }
    RssTables *t = new (std::nothrow) RssTables;
    if (!t) return MTCP_GPU_ENOMEM;
    t->device = device;
    memcpy(t->key, key, 40);
    build_rss_tables(key, t->host);
    if (!HIP_OK(hipMalloc(&t->d, sizeof(t->host)))) {
        delete t;
        return MTCP_GPU_ENOMEM;
    }
    int rc = HIP_OK(hipMemcpyAsync(t->d, t->host, sizeof(t->host), hipMemcpyHostToDevice, st))
                 ? drain(st, Deadline(kOpenWaitUs)) : MTCP_GPU_EIO;
    if (rc != MTCP_GPU_OK) return rc;            // t and its buffer stay (the copy may still run)
    std::lock_guard<std::mutex> lk(rss_mutex());
    rss_cache().push_back(t);
    *out = t->d;
    return MTCP_GPU_OK;
}

// The size hint of a host-side batch: its smallest and largest non-zero
// frame length ({0, 0} when every length is 0).
mtcp_gpu_size_hint size_hint(const mtcp_gpu_desc *desc, uint32_t n) {
    mtcp_gpu_size_hint h = {0xFFFF, 0};
    for (uint32_t i = 0; i < n; ++i)
        if (desc[i].len) h.min_len = std::min(h.min_len, desc[i].len), h.max_len = std::max(h.max_len, desc[i].len);
    if (!h.max_len) h.min_len = 0;
    return h;
}

bool offsets_sorted(const mtcp_gpu_desc *desc, uint32_t n) {
    for (uint32_t i = 1; i < n; ++i)
        if (desc[i].offset < desc[i - 1].offset) return false;
    return true;
}

}  // namespace

extern "C" {

int mtcp_gpu_abi_version(void) { return MTCP_GPU_ABI_VERSION; }

const char *mtcp_gpu_strerror(int err) {
    switch (err) {
        case MTCP_GPU_OK: return "success";
        case MTCP_GPU_EINVAL: return "invalid argument";
        case MTCP_GPU_ENOMEM: return "out of device or pinned host memory";
        case MTCP_GPU_ENODEV: return "no usable HIP device";
        case MTCP_GPU_EIO: return "HIP runtime error";
        case MTCP_GPU_ETIMEDOUT: return "GPU work not finished within the caller's limit";
        default: return "unknown error";
    }
}

int mtcp_gpu_device_count(void) {
    int n = 0;
    if (!HIP_OK(hipGetDeviceCount(&n))) return 0;
    return n;
}

int mtcp_gpu_device_pci_bus_id(int device, char *buf, int len) {
    if (!buf || len < 13) return MTCP_GPU_EINVAL;
    int ndev = 0;
    if (!HIP_OK(hipGetDeviceCount(&ndev)) || device < 0 || device >= ndev) return MTCP_GPU_ENODEV;
    return HIP_OK(hipDeviceGetPCIBusId(buf, len, device)) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

int mtcp_gpu_open(mtcp_gpu_ctx **out, int device, const uint8_t *rss_key, int rss_num_queues,
                  uint32_t flags) {
    static const uint8_t key05[40] = {
        5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5,
        5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5};
    if (!out) return MTCP_GPU_EINVAL;
    *out = nullptr;
    if ((flags & MTCP_GPU_F_RSS) && rss_num_queues < 1) return MTCP_GPU_EINVAL;
    int ndev = 0;
    if (!HIP_OK(hipGetDeviceCount(&ndev)) || device < 0 || device >= ndev) return MTCP_GPU_ENODEV;
    DeviceGuard dg(device);
    if (!dg.ok) return MTCP_GPU_ENODEV;

    mtcp_gpu_ctx *ctx = new (std::nothrow) mtcp_gpu_ctx();
    if (!ctx) return MTCP_GPU_ENOMEM;
    ctx->device = device;
    ctx->flags = flags;
    ctx->rss_nq = (uint32_t)std::max(1, rss_num_queues);
    ctx->rss_endian = (flags & MTCP_GPU_F_RSS_ENDIAN) ? 1u : 0u;
    hipDeviceProp_t prop;
    if (HIP_OK(hipGetDeviceProperties(&prop, device)) && prop.multiProcessorCount > 0)
        ctx->num_cu = prop.multiProcessorCount;

    const uint8_t *key = rss_key ? rss_key : key05;
    for (int i = 0; i < 4; ++i)
        ctx->rss_key_w[i] = ((uint32_t)key[4 * i] << 24) | ((uint32_t)key[4 * i + 1] << 16) |
                            ((uint32_t)key[4 * i + 2] << 8) | (uint32_t)key[4 * i + 3];
    ctx->sched = sched_from_env();
    // one stream per context: its device-resident launches, the host calls
    // that fit one stage and its rxqs all go on it (the context's tables are
    // uploaded on it too, never through the null stream)
    int rc = HIP_OK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) ? MTCP_GPU_OK : MTCP_GPU_ENOMEM;
    if (rc == MTCP_GPU_OK) rc = rss_tables_for(device, key, ctx->stream, &ctx->d_rss_tables);
    if (rc == MTCP_GPU_ETIMEDOUT) {
        ctx->abandoned = true;                   // the upload may still run: leave the stream
        delete ctx;
        return rc;
    }
    if (rc != MTCP_GPU_OK) {
        mtcp_gpu_close(ctx);
        return rc;
    }
    ctx->stage[0].stream = ctx->stream;
    *out = ctx;
    return MTCP_GPU_OK;
}

void mtcp_gpu_close(mtcp_gpu_ctx *ctx) {
    if (!ctx) return;
    DeviceGuard dg(ctx->device);
    if (!ctx->abandoned) {
        // the context's own work finishes first (within its wait limit, if
        // it has one: a device that does not finish it gets the context
        // abandoned instead).  Work the caller queued on its own streams is
        // not waited for: the RSS tables it may read are never freed
        // (rss_tables_for), every other buffer of such a launch is the caller's.
        const Deadline dl(ctx->wait_us);
        for (auto &s : ctx->stage)
            if (s.own_stream && drain(s.stream, dl) == MTCP_GPU_ETIMEDOUT) ctx->abandoned = true;
        if (ctx->stream && drain(ctx->stream, dl) == MTCP_GPU_ETIMEDOUT) ctx->abandoned = true;
    }
    if (ctx->abandoned) {
        // work a timed-out wait gave up on may still copy into the staging:
        // leave every stream and buffer allocated (never touched again)
        // rather than block on a device that stopped answering or free
        // memory under its DMA; only the host-side struct goes
        delete ctx;
        return;
    }
    // every buffer goes back to park.hpp: a free here would wait for the
    // other contexts' work on the device (with a wait limit not even a
    // buffer too large to park is freed)
    const bool may_free = ctx->wait_us == 0;
    for (auto &s : ctx->stage) {
        if (s.own_stream) (void)hipStreamDestroy(s.stream);
        stage_release_buf(s, may_free);
        stage_release_pkts(s, may_free);
        stage_release_host(s, may_free);
        stage_release_opts(s, may_free);
    }
    mtcp_park::release(ctx->h_gather, ctx->h_gather_cap, mtcp_park::kHost, may_free);
    mtcp_park::release(ctx->h_gather_desc, (size_t)ctx->h_gather_desc_cap * sizeof(mtcp_gpu_desc),
                       mtcp_park::kHost, may_free);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int mtcp_gpu_set_wait_limit(mtcp_gpu_ctx *ctx, uint32_t timeout_us) {
    if (!ctx) return MTCP_GPU_EINVAL;
    ctx->wait_us = timeout_us;
    return MTCP_GPU_OK;
}

uint32_t mtcp_gpu_wait_limit(const mtcp_gpu_ctx *ctx) { return ctx ? ctx->wait_us : 0u; }

bool mg_ctx_abandoned(const mtcp_gpu_ctx *ctx) { return ctx && ctx->abandoned; }

int mtcp_gpu_reserve(mtcp_gpu_ctx *ctx, uint64_t max_bytes, uint32_t max_pkts) {
    if (!ctx) return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    DeviceGuard dg(ctx->device);
    if (!dg.ok) return MTCP_GPU_ENODEV;
    const Deadline dl(ctx->wait_us);
    // a host call's batches span at most kStageBytes / kStagePkts and start
    // at stage 0; later stages are used only by calls larger than one stage
    const uint64_t bytes = std::min(max_bytes, kStageBytes);
    const uint32_t pkts = std::min(max_pkts, kStagePkts);
    const int stages = max_bytes == 0 && max_pkts == 0                  ? 0   // kernels only
                       : max_bytes > kStageBytes || max_pkts > kStagePkts ? kStages
                                                                          : 1;
    for (int i = 0; i < stages; ++i) {
        const int rc = stage_reserve(ctx, ctx->stage[i], ((bytes + 15) & ~15ull) + 16, std::max(pkts, 1u), dl);
        if (rc != MTCP_GPU_OK) return rc;
    }
    // a stream sets up its copy queues on its first large copy (7.8 ms
    // measured): do that here for the stages the host calls use, with the
    // pinned buffers a bounded context's calls go through
    const size_t warm = stages ? (size_t)std::min<uint64_t>(ctx->stage[0].buf_cap, 1ull << 20) : 0;
    int rc = MTCP_GPU_OK;
    for (int i = 0; i < stages && rc == MTCP_GPU_OK; ++i) {
        Stage &st = ctx->stage[i];
        rc = stage_host(ctx, st, warm, warm, dl);
        if (rc == MTCP_GPU_OK) {
            memset(st.h_in, 0, warm);
            if (!HIP_OK(hipMemcpyAsync(st.d_buf, st.h_in, warm, hipMemcpyHostToDevice, st.stream)) ||
                !HIP_OK(hipMemcpyAsync(st.h_out, st.d_buf, warm, hipMemcpyDeviceToHost, st.stream)))
                rc = MTCP_GPU_EIO;
        }
    }
    rc = finish_call(ctx, rc, dl, stages);
    if (rc != MTCP_GPU_OK) return rc;
    // the code object loads on the first launch of any of its kernels
    hipFuncAttributes attr;
    if (!HIP_OK(hipFuncGetAttributes(
            &attr, reinterpret_cast<const void *>(
                       &mg::rx_kernel<mg::kRxChunk, false, mg::kSchedSorted, false, 0, 8, 8, true, 6, false>))))
        return MTCP_GPU_EIO;
    return MTCP_GPU_OK;
}

int mtcp_gpu_dev_ioctl(mtcp_gpu_ctx *ctx, int nif, int cmd, void *argp) {
    (void)nif;
    (void)argp;
    if (!ctx) return -1;
    switch (cmd) {   // the commands this device computes (dpdk_module.c:809-816 contract)
        case MTCP_GPU_PKT_RX_IP_CSUM:
        case MTCP_GPU_PKT_RX_TCP_CSUM:
        case MTCP_GPU_PKT_TX_IP_CSUM:
        case MTCP_GPU_PKT_TX_TCPIP_CSUM:
            return 0;
        default:
            return -1;
    }
}

void *mtcp_gpu_stream(mtcp_gpu_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

uint32_t mtcp_gpu_record_size(const mtcp_gpu_ctx *ctx) { return ctx ? (uint32_t)record_size(ctx) : 0u; }

const char *mtcp_gpu_last_kernel(const mtcp_gpu_ctx *ctx) { return ctx ? ctx->last_kernel : ""; }

int mtcp_gpu_sync(mtcp_gpu_ctx *ctx) {
    if (!ctx) return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    DeviceGuard dg(ctx->device);
    // with a wait limit: MTCP_GPU_ETIMEDOUT past it, and the context stays
    // usable (what is still running is the caller's own device work)
    return drain(ctx->stream, Deadline(ctx->wait_us));
}

int mtcp_gpu_rx_chunk_flow_dev(mtcp_gpu_ctx *ctx, const void *d_buf, uint64_t buf_len,
                               const mtcp_gpu_desc *d_desc, uint32_t n, uint32_t off_shift,
                               mtcp_gpu_result *d_out, uint32_t *d_bins, void *stream) {
    return mtcp_gpu_rx_chunk_hint_dev(ctx, d_buf, buf_len, d_desc, n, off_shift, d_out, d_bins, nullptr, stream);
}

int mtcp_gpu_rx_chunk_hint_dev(mtcp_gpu_ctx *ctx, const void *d_buf, uint64_t buf_len,
                               const mtcp_gpu_desc *d_desc, uint32_t n, uint32_t off_shift,
                               mtcp_gpu_result *d_out, uint32_t *d_bins, const mtcp_gpu_size_hint *hint,
                               void *stream) {
    if (!ctx || (n && (!d_buf || !d_desc || !d_out)) || off_shift > 16 || (buf_len & 15) ||
        ((uintptr_t)d_buf & 15) || ((uintptr_t)d_out & out_align(ctx)) || ((uintptr_t)d_desc & 7) ||
        ((uintptr_t)d_bins & 3))
        return MTCP_GPU_EINVAL;
    DeviceGuard dg(ctx->device);
    mg::KParams kp = base_params(ctx);
    kp.buf = static_cast<const uint8_t *>(d_buf);
    kp.buf_len = buf_len;
    kp.desc = d_desc;
    kp.n = n;
    kp.off_shift = off_shift;
    kp.out = d_out;
    kp.bins = d_bins;
    return launch<mg::kRxChunk>(ctx, kp, pick(ctx, stream), hint);
}

int mtcp_gpu_rx_chunk_dev(mtcp_gpu_ctx *ctx, const void *d_buf, uint64_t buf_len,
                          const mtcp_gpu_desc *d_desc, uint32_t n, uint32_t off_shift,
                          mtcp_gpu_result *d_out, void *stream) {
    return mtcp_gpu_rx_chunk_flow_dev(ctx, d_buf, buf_len, d_desc, n, off_shift, d_out, nullptr, stream);
}

int mtcp_gpu_rx_ptrs_flow_dev(mtcp_gpu_ctx *ctx, const uint8_t *const *d_pkts, const uint16_t *d_lens,
                              uint32_t n, mtcp_gpu_result *d_out, uint32_t *d_bins, void *stream) {
    if (!ctx || (n && (!d_pkts || !d_lens || !d_out)) || ((uintptr_t)d_out & out_align(ctx)) ||
        ((uintptr_t)d_bins & 3))
        return MTCP_GPU_EINVAL;
    DeviceGuard dg(ctx->device);
    mg::KParams kp = base_params(ctx);
    kp.ptrs = d_pkts;
    kp.lens = d_lens;
    kp.n = n;
    kp.out = d_out;
    kp.bins = d_bins;
    return launch<mg::kRxPtrs>(ctx, kp, pick(ctx, stream));
}

int mtcp_gpu_rx_ptrs_dev(mtcp_gpu_ctx *ctx, const uint8_t *const *d_pkts, const uint16_t *d_lens,
                         uint32_t n, mtcp_gpu_result *d_out, void *stream) {
    return mtcp_gpu_rx_ptrs_flow_dev(ctx, d_pkts, d_lens, n, d_out, nullptr, stream);
}

int mtcp_gpu_tx_fill_ptrs_dev(mtcp_gpu_ctx *ctx, uint8_t *const *d_pkts, const uint16_t *d_lens,
                              uint32_t n, void *stream) {
    if (!ctx || (n && (!d_pkts || !d_lens))) return MTCP_GPU_EINVAL;
    DeviceGuard dg(ctx->device);
    mg::KParams kp = base_params(ctx);
    kp.ptrs = reinterpret_cast<const uint8_t *const *>(d_pkts);
    kp.lens = d_lens;
    kp.n = n;
    return launch<mg::kTxPtrs>(ctx, kp, pick(ctx, stream));
}

int mtcp_gpu_tx_fill_dev(mtcp_gpu_ctx *ctx, void *d_buf, uint64_t buf_len,
                         const mtcp_gpu_desc *d_desc, uint32_t n, uint32_t off_shift,
                         void *stream) {
    if (!ctx || (n && (!d_buf || !d_desc)) || off_shift > 16 || (buf_len & 15) ||
        ((uintptr_t)d_buf & 15) || ((uintptr_t)d_desc & 7))
        return MTCP_GPU_EINVAL;
    DeviceGuard dg(ctx->device);
    mg::KParams kp = base_params(ctx);
    kp.buf = static_cast<const uint8_t *>(d_buf);
    kp.buf_len = buf_len;
    kp.desc = d_desc;
    kp.n = n;
    kp.off_shift = off_shift;
    return launch<mg::kTxChunk>(ctx, kp, pick(ctx, stream));
}

}  // extern "C"

namespace {

// Host-memory rx (mtcp_gpu_rx_chunk, _rx_ptrs): batches of packets stream
// through kStages stages — stage 0 on the context's stream, 1 and 2 on their
// own — so that the H2D of batch b+1 overlaps the kernel of b and the D2H of
// b-1.  Each batch copies only the byte span its packets occupy and the
// kernel rebases descriptor offsets by that span's start.  The contract of
// host_call.hpp per stage: a bounded call bounces every byte through the
// stage's pinned buffers (`owned`: buf / desc already are the context's own
// pinned gather and are not copied again).
//
// One batch on stage s, its frames already on their way into s.d_buf: the
// descriptors up, the rx launch, for mtcp_gpu_rx_chunk_opts the option kernel
// over the same frames and the records rx just wrote, then the records (and
// option records) down — to out (opts), or for a bounded call into the stage's
// bounce buffers, owed to the caller once the stage has drained.
int rx_batch(mtcp_gpu_ctx *ctx, Stage &s, mg::KParams kp, const void *dsrc,
             const mtcp_gpu_size_hint &hint, uint8_t *out, mtcp_gpu_tcpopt *opts, bool bounce) {
    const size_t rbytes = kp.n * (size_t)record_size(kp), obytes = (size_t)kp.n * sizeof(mtcp_gpu_tcpopt);
    kp.desc = s.d_desc;
    kp.out = s.d_out;
    int rc = HIP_OK(hipMemcpyAsync(s.d_desc, dsrc, (size_t)kp.n * sizeof(mtcp_gpu_desc), hipMemcpyHostToDevice,
                                   s.stream)) ? MTCP_GPU_OK : MTCP_GPU_EIO;
    if (rc == MTCP_GPU_OK) rc = launch<mg::kRxChunk>(ctx, kp, s.stream, &hint);
    if (rc == MTCP_GPU_OK && opts) rc = stage_opts(s, bounce);
    if (rc == MTCP_GPU_OK && opts) rc = launch_tcpopt<false>(ctx, kp, s.d_out, s.d_opt, s.stream);
    if (rc == MTCP_GPU_OK &&
        ((opts && !HIP_OK(hipMemcpyAsync(bounce ? s.h_opt : opts, s.d_opt, obytes, hipMemcpyDeviceToHost, s.stream))) ||
         !HIP_OK(hipMemcpyAsync(bounce ? s.h_out : out, s.d_out, rbytes, hipMemcpyDeviceToHost, s.stream))))
        rc = MTCP_GPU_EIO;
    if (rc == MTCP_GPU_OK && bounce) {
        stage_pend(s, out, s.h_out, rbytes);
        if (opts) stage_pend(s, opts, s.h_opt, obytes);
    }
    return rc;
}

int rx_host(mtcp_gpu_ctx *ctx, const uint8_t *buf, uint64_t buf_len, const mtcp_gpu_desc *desc, uint32_t n,
            uint32_t off_shift, mtcp_gpu_result *out, bool owned, const Deadline &dl,
            mtcp_gpu_tcpopt *opts = nullptr) {
    int rc = MTCP_GPU_OK;
    uint8_t *const out_b = reinterpret_cast<uint8_t *>(out);
    const size_t rec = (size_t)record_size(ctx);
    const bool bounce = dl.bounded;
    const uint64_t out_bytes = (uint64_t)kStagePkts * rec;
    mg::KParams kp = base_params(ctx);
    kp.off_shift = off_shift;
    if (!offsets_sorted(desc, n)) {
        // arbitrary order: stage the whole chunk once, then batches of descriptors
        Stage &s = ctx->stage[0];
        const uint64_t padded = (buf_len + 15) & ~15ull;
        rc = stage_reserve(ctx, s, padded + 16, kStagePkts, dl);
        if (rc == MTCP_GPU_OK && bounce)
            rc = stage_host(ctx, s, owned ? 0 : padded + (uint64_t)kStagePkts * sizeof(mtcp_gpu_desc), out_bytes, dl);
        const uint8_t *src = buf;
        if (rc == MTCP_GPU_OK && bounce && !owned) {
            bounce_in(s.h_in, buf, buf_len);
            src = s.h_in;
        }
        if (rc == MTCP_GPU_OK && !HIP_OK(hipMemcpyAsync(s.d_buf, src, buf_len, hipMemcpyHostToDevice, s.stream)))
            rc = MTCP_GPU_EIO;
        kp.buf = s.d_buf;
        kp.buf_len = buf_len;
        for (uint32_t first = 0; first < n && rc == MTCP_GPU_OK; first += kStagePkts) {
            kp.n = std::min(n - first, kStagePkts);
            if ((rc = stage_collect(ctx, s, dl)) != MTCP_GPU_OK) break;   // the previous batch
            const void *dsrc = desc + first;
            if (bounce && !owned) dsrc = memcpy(s.h_in + padded, desc + first, (size_t)kp.n * sizeof(mtcp_gpu_desc));
            rc = rx_batch(ctx, s, kp, dsrc, size_hint(desc + first, kp.n), out_b + first * rec,
                          opts ? opts + first : nullptr, bounce);
        }
    } else {
        uint32_t first = 0;
        for (int b = 0; first < n && rc == MTCP_GPU_OK; ++b) {
            // grow the batch while its byte span fits one stage
            const uint64_t lo = std::min(((uint64_t)desc[first].offset << off_shift) & ~15ull,
                                         buf_len & ~15ull);
            uint64_t hi = lo;
            uint32_t cnt = 0;
            mtcp_gpu_size_hint hint = {0xFFFF, 0};
            while (first + cnt < n && cnt < kStagePkts) {
                const uint64_t p = (uint64_t)desc[first + cnt].offset << off_shift;
                const uint16_t len = desc[first + cnt].len;
                const uint64_t end = std::max(std::min(p + len, buf_len), lo);
                if (cnt > 0 && std::max(hi, end) - lo > kStageBytes) break;
                hi = std::max(hi, end);
                if (len) hint.min_len = std::min(hint.min_len, len), hint.max_len = std::max(hint.max_len, len);
                ++cnt;
            }
            if (!hint.max_len) hint.min_len = 0;
            Stage &s = ctx->stage[b % kStages];
            const uint64_t span = hi - lo, padded = (span + 15) & ~15ull;
            if ((rc = stage_collect(ctx, s, dl)) != MTCP_GPU_OK) break;   // its batch b - kStages
            rc = stage_reserve(ctx, s, padded + 16, kStagePkts, dl);
            if (rc == MTCP_GPU_OK && bounce)
                rc = stage_host(ctx, s, owned ? 0 : padded + (uint64_t)cnt * sizeof(mtcp_gpu_desc), out_bytes, dl);
            if (rc != MTCP_GPU_OK) break;
            const uint8_t *src = buf + lo;
            const void *dsrc = desc + first;
            if (bounce && !owned) {
                bounce_in(s.h_in, buf + lo, span);
                src = s.h_in;
                dsrc = memcpy(s.h_in + padded, desc + first, (size_t)cnt * sizeof(mtcp_gpu_desc));
            }
            kp.buf = s.d_buf;
            kp.buf_len = span;           // descriptors are bounded by the caller's buf_len
            kp.base_sub = (int64_t)lo;
            kp.n = cnt;
            if (span && !HIP_OK(hipMemcpyAsync(s.d_buf, src, span, hipMemcpyHostToDevice, s.stream)))
                rc = MTCP_GPU_EIO;
            if (rc == MTCP_GPU_OK)
                rc = rx_batch(ctx, s, kp, dsrc, hint, out_b + first * rec, opts ? opts + first : nullptr, bounce);
            first += cnt;
        }
    }
    // (a stage_collect that timed out has abandoned the context already: no
    // more waits then, and no stage's records are copied out)
    return finish_call(ctx, rc, dl, kStages);
}

// Gather a pointer burst into the context's pinned PSIO-style chunk (64 B
// aligned slots, pslib.c:146) with its descriptors; *total = chunk bytes.
int gather_burst(mtcp_gpu_ctx *ctx, const uint8_t *const *pkts, const uint16_t *lens, uint32_t n,
                 uint64_t *total_out, const Deadline &dl) {
    if (ctx->abandoned) return MTCP_GPU_EIO;     // its staging may still be under DMA
    const bool may_free = !dl.bounded;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) total += ((uint64_t)lens[i] + 63) & ~63ull;
    if (total > ctx->h_gather_cap) {
        mtcp_park::release(ctx->h_gather, ctx->h_gather_cap, mtcp_park::kHost, may_free);
        ctx->h_gather = nullptr;
        ctx->h_gather_cap = 0;
        if (!HIP_OK(mtcp_park::alloc(&ctx->h_gather, total, mtcp_park::kHost))) return MTCP_GPU_ENOMEM;
        ctx->h_gather_cap = total;
    }
    if (n > ctx->h_gather_desc_cap) {
        mtcp_park::release(ctx->h_gather_desc, (size_t)ctx->h_gather_desc_cap * sizeof(mtcp_gpu_desc),
                           mtcp_park::kHost, may_free);
        ctx->h_gather_desc = nullptr;
        ctx->h_gather_desc_cap = 0;
        if (!HIP_OK(mtcp_park::alloc(&ctx->h_gather_desc, (size_t)n * sizeof(mtcp_gpu_desc), mtcp_park::kHost)))
            return MTCP_GPU_ENOMEM;
        ctx->h_gather_desc_cap = n;
    }
    uint64_t off = 0;
    for (uint32_t i = 0; i < n; ++i) {
        mtcp_gpu_desc &d = ctx->h_gather_desc[i];
        d.offset = (uint32_t)(off >> 6);
        d.len = lens[i];
        d.flags = d.rsvd = 0;
        if (pkts[i]) stage_copy(ctx->h_gather + off, pkts[i], lens[i]);
        else d.len = 0xFFFF, d.offset = 0xFFFFFFFFu;   // -> BAD_DESC
        off += ((uint64_t)lens[i] + 63) & ~63ull;
    }
    stage_fence();
    *total_out = total;
    return MTCP_GPU_OK;
}

// The tx fill of the host calls: over the n frames staged in s.d_buf by the
// descriptors in s.d_desc, reporting {checks, T} per frame into s.d_out.
int launch_tx_report(mtcp_gpu_ctx *ctx, Stage &s, uint64_t buf_len, uint32_t n, uint32_t off_shift) {
    mg::KParams kp = base_params(ctx);
    kp.buf = s.d_buf;
    kp.buf_len = buf_len;
    kp.desc = s.d_desc;
    kp.n = n;
    kp.off_shift = off_shift;
    kp.tx_report = reinterpret_cast<uint2 *>(s.d_out);                // n x 8 B <= n x 40 B
    return launch<mg::kTxChunk>(ctx, kp, s.stream);
}

// The two check fields of a filled frame (the tx kernels' report: {ip check
// | tcp check << 16, T}, T the TCP header's offset, 0 = not filled), written
// by the calling thread: iph->check (ip_out.c:164), tcph->check (tcp_out.c:329)
inline void write_checks(uint8_t *frame, uint2 r) {
    const uint16_t ipc = (uint16_t)r.x, tcpc = (uint16_t)(r.x >> 16);
    memcpy(frame + 24, &ipc, 2);
    memcpy(frame + r.y + 16, &tcpc, 2);
}

}  // namespace

extern "C" {

int mtcp_gpu_rx_chunk(mtcp_gpu_ctx *ctx, const uint8_t *buf, uint64_t buf_len,
                      const mtcp_gpu_desc *desc, uint32_t n, uint32_t off_shift,
                      mtcp_gpu_result *out) {
    if (!ctx || (n && (!buf || !desc || !out)) || off_shift > 16) return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    return rx_host(ctx, buf, buf_len, desc, n, off_shift, out, false, Deadline(ctx->wait_us));
}

int mtcp_gpu_rx_chunk_opts(mtcp_gpu_ctx *ctx, const uint8_t *buf, uint64_t buf_len,
                           const mtcp_gpu_desc *desc, uint32_t n, uint32_t off_shift,
                           mtcp_gpu_result *out, mtcp_gpu_tcpopt *opts) {
    if (!ctx || (n && (!buf || !desc || !out || !opts)) || off_shift > 16) return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    return rx_host(ctx, buf, buf_len, desc, n, off_shift, out, false, Deadline(ctx->wait_us), opts);
}

int mtcp_gpu_rx_ptrs(mtcp_gpu_ctx *ctx, const uint8_t *const *pkts, const uint16_t *lens,
                     uint32_t n, mtcp_gpu_result *out) {
    if (!ctx || (n && (!pkts || !lens || !out))) return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    uint64_t total = 0;
    const int rc = gather_burst(ctx, pkts, lens, n, &total, dl);
    if (rc != MTCP_GPU_OK) return rc;
    return rx_host(ctx, ctx->h_gather, total, ctx->h_gather_desc, n, 6, out, true, dl);
}

// tx fill of a host pointer burst (a DPDK wmbufs[].m_table, dpdk_module.c:341-370):
// the frames are gathered into pinned staging and checked on the GPU, which
// reports {checks, T} per frame (the tx kernels' report mode); only the two
// check fields are written back into the caller's frames, here on the host,
// once the report is in (within timeout_us, else the context's wait limit;
// past it nothing has been written into the caller's frames).  mTCP's own tx
// fill never waits on a device (tcp_out.c:320-329, ip_out.c:147-165, run from
// RunMainLoop core.c:818-824): the caller fills the frames itself.
int mtcp_gpu_tx_fill_ptrs_for(mtcp_gpu_ctx *ctx, uint8_t *const *pkts, const uint16_t *lens, uint32_t n,
                              uint32_t *n_filled, uint32_t timeout_us) {
    if (!ctx || (n && (!pkts || !lens))) return MTCP_GPU_EINVAL;
    if (n_filled) *n_filled = 0;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    const Deadline dl(timeout_us ? timeout_us : ctx->wait_us);
    uint64_t total = 0;
    int rc = gather_burst(ctx, pkts, lens, n, &total, dl);
    if (rc != MTCP_GPU_OK) return rc;
    Stage &s = ctx->stage[0];
    rc = stage_reserve(ctx, s, ((total + 15) & ~15ull) + 16, n, dl);
    if (rc != MTCP_GPU_OK) return rc;
    uint2 *report = reinterpret_cast<uint2 *>(ctx->h_gather_desc);    // reused once the H2D is done
    static_assert(sizeof(uint2) == sizeof(mtcp_gpu_desc), "report reuses the descriptor staging");
    // both ends of every copy are the context's own: the pinned gather up,
    // the report down into the descriptors' place
    Call hc(s, dl, {ctx, dl});
    hc.h2d(s.d_buf, ctx->h_gather, total);
    hc.h2d(s.d_desc, ctx->h_gather_desc, (size_t)n * sizeof(mtcp_gpu_desc));
    if (hc.ok()) hc.note(launch_tx_report(ctx, s, total, n, 6));
    hc.d2h(report, s.d_out, (size_t)n * sizeof(uint2));
    if ((rc = hc.finish()) != MTCP_GPU_OK) return rc;
    uint32_t cnt = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!report[i].y) continue;
        write_checks(pkts[i], report[i]);
        ++cnt;
    }
    if (n_filled) *n_filled = cnt;
    return MTCP_GPU_OK;
}

int mtcp_gpu_tx_fill_ptrs(mtcp_gpu_ctx *ctx, uint8_t *const *pkts, const uint16_t *lens, uint32_t n,
                          uint32_t *n_filled) {
    return mtcp_gpu_tx_fill_ptrs_for(ctx, pkts, lens, n, n_filled, 0);
}

// tx fill of a host chunk, in place: the chunk goes to the GPU once, the
// kernel reports {checks, T} per frame (n x 8 B back instead of the whole
// chunk) and the calling thread writes the two check fields of each filled
// frame.  Stages the chunk and the descriptors; the report comes down pinned,
// and nothing is written into the chunk unless it came in time.
int mtcp_gpu_tx_fill(mtcp_gpu_ctx *ctx, uint8_t *buf, uint64_t buf_len, const mtcp_gpu_desc *desc,
                     uint32_t n, uint32_t off_shift, uint32_t *n_filled) {
    if (!ctx || (n && (!buf || !desc)) || off_shift > 16) return MTCP_GPU_EINVAL;
    if (n_filled) *n_filled = 0;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    Stage &s = ctx->stage[0];
    const uint64_t padded = (buf_len + 15) & ~15ull;
    const uint64_t dbytes = (uint64_t)n * sizeof(mtcp_gpu_desc);
    int rc = stage_reserve(ctx, s, padded + 16, n, dl);
    if (rc == MTCP_GPU_OK)
        rc = stage_host(ctx, s, dl.bounded ? padded + dbytes : 0, (uint64_t)n * sizeof(uint2), dl);
    if (rc != MTCP_GPU_OK) return rc;
    Call hc(s, dl, {ctx, dl});
    // the 16 B past the chunk (the kernels' last vector load of a frame
    // ending there) read as zeros
    if (!HIP_OK(hipMemsetAsync(s.d_buf + (buf_len & ~15ull), 0, 16, s.stream))) hc.note(MTCP_GPU_EIO);
    hc.up(s.d_buf, buf, buf_len, true);
    hc.up(s.d_desc, desc, dbytes);
    if (hc.ok()) hc.note(launch_tx_report(ctx, s, buf_len, n, off_shift));   // descriptor bound: the caller's length
    const uint2 *report = reinterpret_cast<const uint2 *>(hc.down_pinned(s.d_out, (uint64_t)n * sizeof(uint2)));
    if ((rc = hc.finish()) != MTCP_GPU_OK) return rc;
    uint32_t cnt = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t off = (uint64_t)desc[i].offset << off_shift;
        // the kernel reports only frames inside the chunk (checked again here)
        if (!report[i].y || off + report[i].y + 18 > buf_len) continue;
        write_checks(buf + off, report[i]);
        ++cnt;
    }
    if (n_filled) *n_filled = cnt;
    return MTCP_GPU_OK;
}

// ---- TCP option records -------------------------------------
int mtcp_gpu_rx_tcpopt_chunk_dev(mtcp_gpu_ctx *ctx, const void *d_buf, uint64_t buf_len,
                                 const mtcp_gpu_desc *d_desc, uint32_t n, uint32_t off_shift,
                                 const mtcp_gpu_result *d_res, mtcp_gpu_tcpopt *d_opt, void *stream) {
    if (!ctx || (n && (!d_buf || !d_desc || !d_res || !d_opt)) || off_shift > 16 || (buf_len & 15) ||
        ((uintptr_t)d_buf & 15) || ((uintptr_t)d_res & out_align(ctx)) || ((uintptr_t)d_desc & 7) ||
        ((uintptr_t)d_opt & 15))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    mg::KParams kp = base_params(ctx);
    kp.buf = static_cast<const uint8_t *>(d_buf);
    kp.buf_len = buf_len;
    kp.desc = d_desc;
    kp.n = n;
    kp.off_shift = off_shift;
    return launch_tcpopt<false>(ctx, kp, d_res, d_opt, pick(ctx, stream));
}

int mtcp_gpu_rx_tcpopt_ptrs_dev(mtcp_gpu_ctx *ctx, const uint8_t *const *d_pkts, const uint16_t *d_lens,
                                uint32_t n, const mtcp_gpu_result *d_res, mtcp_gpu_tcpopt *d_opt,
                                void *stream) {
    if (!ctx || (n && (!d_pkts || !d_lens || !d_res || !d_opt)) || ((uintptr_t)d_res & out_align(ctx)) ||
        ((uintptr_t)d_pkts & 7) || ((uintptr_t)d_lens & 1) || ((uintptr_t)d_opt & 15))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    mg::KParams kp = base_params(ctx);
    kp.ptrs = d_pkts;
    kp.lens = d_lens;
    kp.n = n;
    return launch_tcpopt<true>(ctx, kp, d_res, d_opt, pick(ctx, stream));
}

// ---- flow-table hash --------------------------------------
int mtcp_gpu_flow_hash_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_result *d_res, uint32_t n,
                           uint32_t *d_bins, void *stream) {
    if (!ctx || (n && (!d_res || !d_bins)) || ((uintptr_t)d_res & 7) || ((uintptr_t)d_bins & 3) ||
        (ctx->flags & MTCP_GPU_F_COMPACT))          // reads 40 B records (the 4-tuple)
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    const uint32_t blocks = std::min<uint32_t>((n + mg::kBlock - 1) / mg::kBlock,
                                               (uint32_t)ctx->num_cu * 8);
    hipLaunchKernelGGL(mg::flow_hash_kernel, dim3(blocks), dim3(mg::kBlock), 0, pick(ctx, stream),
                       d_res, n, d_bins);
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

// The records go up into stage 0's record buffer; its chunk buffer holds bins[n].
int mtcp_gpu_flow_hash(mtcp_gpu_ctx *ctx, const mtcp_gpu_result *res, uint32_t n,
                       uint32_t *bins) {
    if (!ctx || (n && (!res || !bins)) || (ctx->flags & MTCP_GPU_F_COMPACT)) return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    const uint64_t rbytes = (uint64_t)n * sizeof(mtcp_gpu_result), bbytes = (uint64_t)n * sizeof(uint32_t);
    Stage &s = ctx->stage[0];
    int rc = stage_reserve(ctx, s, bbytes, n, dl);
    if (rc == MTCP_GPU_OK && dl.bounded) rc = stage_host(ctx, s, rbytes, bbytes, dl);
    if (rc != MTCP_GPU_OK) return rc;
    uint32_t *d_bins = reinterpret_cast<uint32_t *>(s.d_buf);
    Call hc(s, dl, {ctx, dl});
    hc.up(s.d_out, res, rbytes);
    if (hc.ok()) hc.note(mtcp_gpu_flow_hash_dev(ctx, s.d_out, n, d_bins, s.stream));
    hc.down(bins, d_bins, bbytes);
    return hc.finish();
}

// ---- steering by RSS queue ----------------------------------
namespace {

static_assert(mg::kSteerMaxLists == MTCP_GPU_STEER_MAX_QUEUES + 1, "steer_kernels.hpp sizes its LDS for the ABI's Q");

uint32_t steer_queues(const mtcp_gpu_ctx *ctx) { return (ctx->flags & MTCP_GPU_F_RSS) ? ctx->rss_nq : 1u; }

// The workspace of a batch above one tile: the parked destination bytes, the
// counts of every list for every wave of every tile (list-major, four waves
// per tile) and the lists' totals, each part 16 B aligned.  A batch of one tile runs in one workgroup and uses none.
struct SteerWork {
    uint32_t ntiles;
    uint64_t cnt_off, tot_off, bytes;
};
SteerWork steer_work(uint32_t Q, uint32_t n) {
    SteerWork w{};
    w.ntiles = (n + mg::kSteerTile - 1) / mg::kSteerTile;
    if (w.ntiles <= 1) {
        w.bytes = 16;
        return w;
    }
    const uint64_t L = (uint64_t)Q + 1;
    w.cnt_off = ((uint64_t)n + 15) & ~15ull;
    w.tot_off = w.cnt_off + 16 * L * w.ntiles;
    w.bytes = w.tot_off + ((4 * L + 15) & ~15ull);
    return w;
}

}  // namespace

uint32_t mtcp_gpu_steer_tile(void) { return mg::kSteerTile; }

uint64_t mtcp_gpu_steer_work_bytes(const mtcp_gpu_ctx *ctx, uint32_t n) {
    if (!ctx || n > MTCP_GPU_STEER_MAX_PKTS || steer_queues(ctx) > MTCP_GPU_STEER_MAX_QUEUES) return 0;
    return steer_work(steer_queues(ctx), n).bytes;
}

int mtcp_gpu_steer_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_result *d_res, uint32_t n, uint32_t flags,
                       uint32_t *d_idx, uint32_t *d_start, const mtcp_gpu_desc *d_desc,
                       mtcp_gpu_desc *d_desc_out, void *d_work, uint64_t work_bytes, void *stream) {
    if (!ctx || (flags & ~MTCP_GPU_STEER_DROP_BAD) || n > MTCP_GPU_STEER_MAX_PKTS ||
        steer_queues(ctx) > MTCP_GPU_STEER_MAX_QUEUES || (n && (!d_res || !d_idx || !d_start || !d_work)) ||
        (!d_desc != !d_desc_out) || ((uintptr_t)d_res & 7) || ((uintptr_t)d_idx & 3) ||
        ((uintptr_t)d_start & 3) || ((uintptr_t)d_desc & 7) || ((uintptr_t)d_desc_out & 7) ||
        ((uintptr_t)d_work & 15))
        return MTCP_GPU_EINVAL;
    const uint32_t Q = steer_queues(ctx);
    const SteerWork w = steer_work(Q, n);
    if (n && work_bytes < w.bytes) return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    hipStream_t st = pick(ctx, stream);
    const bool cmp = ctx->flags & MTCP_GPU_F_COMPACT, gather = d_desc != nullptr;
    const uint32_t *res = reinterpret_cast<const uint32_t *>(d_res);
    const uint2 *desc = reinterpret_cast<const uint2 *>(d_desc);
    uint2 *desc_out = reinterpret_cast<uint2 *>(d_desc_out);
    const dim3 block(mg::kBlock);
    if (w.ntiles == 1) {
#define STEER_ONE(C, G) \
    hipLaunchKernelGGL((mg::steer_one_kernel<C, G>), dim3(1), block, 0, st, res, n, Q, flags, d_idx, d_start, \
                       desc, desc_out)
        if (cmp) {
            if (gather) STEER_ONE(true, true); else STEER_ONE(true, false);
        } else {
            if (gather) STEER_ONE(false, true); else STEER_ONE(false, false);
        }
#undef STEER_ONE
        return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
    }
    uint8_t *work = static_cast<uint8_t *>(d_work);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(work + w.cnt_off);
    uint32_t *totals = reinterpret_cast<uint32_t *>(work + w.tot_off);
    if (cmp)
        hipLaunchKernelGGL(mg::steer_count_kernel<true>, dim3(w.ntiles), block, 0, st, res, n, Q, flags, work,
                           cnt, w.ntiles);
    else
        hipLaunchKernelGGL(mg::steer_count_kernel<false>, dim3(w.ntiles), block, 0, st, res, n, Q, flags, work,
                           cnt, w.ntiles);
    hipLaunchKernelGGL(mg::steer_scan_kernel, dim3(Q + 1), block, 0, st, cnt,
                       w.ntiles * mg::kWavesPerBlock, totals);
    if (gather)
        hipLaunchKernelGGL(mg::steer_emit_kernel<true>, dim3(w.ntiles), block, 0, st, work, n, Q, cnt, totals,
                           w.ntiles, d_idx, d_start, desc, desc_out);
    else
        hipLaunchKernelGGL(mg::steer_emit_kernel<false>, dim3(w.ntiles), block, 0, st, work, n, Q, cnt, totals,
                           w.ntiles, d_idx, d_start, desc, desc_out);
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

int mtcp_gpu_steer(mtcp_gpu_ctx *ctx, const mtcp_gpu_result *res, uint32_t n, uint32_t flags,
                   uint32_t *idx, uint32_t *start) {
    if (!ctx || (flags & ~MTCP_GPU_STEER_DROP_BAD) || n > MTCP_GPU_STEER_MAX_PKTS ||
        steer_queues(ctx) > MTCP_GPU_STEER_MAX_QUEUES || (n && (!res || !idx || !start)))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    const uint32_t Q = steer_queues(ctx);
    const SteerLayout l(n, Q, record_size(ctx), steer_work(Q, n).bytes);
    Stage &s = ctx->stage[0];
    int rc = stage_reserve(ctx, s, l.dev_bytes, n, dl);
    if (rc == MTCP_GPU_OK && dl.bounded) rc = stage_host(ctx, s, l.in_bytes, l.out_bytes(), dl);
    if (rc != MTCP_GPU_OK) return rc;
    Call hc(s, dl, {ctx, dl});
    hc.up(s.d_out, res, n * record_size(ctx));
    if (hc.ok())
        hc.note(mtcp_gpu_steer_dev(ctx, s.d_out, n, flags, l.idx(s), l.start(s), nullptr, nullptr, l.work(s),
                                   l.work.bytes, s.stream));
    hc.down2(idx, l.idx(s), l.idx.bytes, start, l.start.bytes);
    return hc.finish();
}

// ---- grouping by stream --------------------------------------
static_assert(MTCP_GPU_GROUP_MAX_PKTS == MTCP_GPU_FLOWTAB_MAX_BATCH, "a lookup's whole batch can be grouped");

uint32_t mtcp_gpu_group_tile(void) { return mg::kGroupTile; }

uint64_t mtcp_gpu_group_work_bytes(uint32_t n, uint32_t max_id) {
    if (n > MTCP_GPU_GROUP_MAX_PKTS || max_id > MTCP_GPU_FLOWTAB_MAX_ID) return 0;
    return mg::group_work(n, max_id).bytes;
}

int mtcp_gpu_group_dev(mtcp_gpu_ctx *ctx, const uint32_t *d_sid, uint32_t n, uint32_t max_id,
                       uint32_t *d_idx, uint32_t *d_seg_sid, uint32_t *d_seg_start, uint32_t *d_nseg,
                       void *d_work, uint64_t work_bytes, void *stream) {
    if (!ctx || n > MTCP_GPU_GROUP_MAX_PKTS || max_id > MTCP_GPU_FLOWTAB_MAX_ID ||
        (n && (!d_sid || !d_idx || !d_seg_sid || !d_seg_start || !d_nseg || !d_work)) ||
        ((uintptr_t)d_sid & 3) || ((uintptr_t)d_idx & 3) || ((uintptr_t)d_seg_sid & 3) ||
        ((uintptr_t)d_seg_start & 3) || ((uintptr_t)d_nseg & 3) || ((uintptr_t)d_work & 15))
        return MTCP_GPU_EINVAL;
    const mg::GroupWork w = mg::group_work(n, max_id);
    if (n && work_bytes < w.bytes) return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    hipStream_t st = pick(ctx, stream);
    const dim3 block(mg::kBlock), tiles(w.ntiles);
    if (w.one) {
        hipLaunchKernelGGL(mg::group_one_kernel, dim3(1), block, 0, st, d_sid, n, max_id, d_idx, d_seg_sid,
                           d_seg_start, d_nseg);
        return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
    }
    uint8_t *work = static_cast<uint8_t *>(d_work);
    auto at = [&](uint64_t off) { return reinterpret_cast<uint32_t *>(work + off); };
    uint32_t *cnt = at(w.cnt_off), *totals = at(w.tot_off), *segcnt = at(w.seg_off), *segtot = at(w.segtot_off);
    // pass p reads the pairs pass p - 1 wrote (pass 0: d_sid, the index is the
    // position) and writes keys to key[p & 1], indices to idx[p & 1] or d_idx
    const uint32_t *src_key = d_sid, *src_idx = nullptr;
    for (uint32_t p = 0; p < w.passes; ++p) {
        const mg::GroupDigit d = mg::group_digit(w.key_bits, w.passes, p);
        uint32_t *dst_key = at(w.key_off[p & 1]);
        uint32_t *dst_idx = p + 1 == w.passes ? d_idx : at(w.idx_off[p & 1]);
        if (p == 0)
            hipLaunchKernelGGL(mg::group_count_kernel<true>, tiles, block, 0, st, src_key, n, max_id, d.shift, d.bits,
                               cnt, w.ntiles);
        else
            hipLaunchKernelGGL(mg::group_count_kernel<false>, tiles, block, 0, st, src_key, n, max_id, d.shift,
                               d.bits, cnt, w.ntiles);
        hipLaunchKernelGGL(mg::group_scan_kernel, dim3(1u << d.bits), block, 0, st, reinterpret_cast<uint4 *>(cnt),
                           w.ntiles, totals);
        if (p == 0)
            hipLaunchKernelGGL(mg::group_emit_kernel<true>, tiles, block, 0, st, src_key, src_idx, n, max_id, d.shift,
                               d.bits, cnt, totals, w.ntiles, dst_key, dst_idx);
        else
            hipLaunchKernelGGL(mg::group_emit_kernel<false>, tiles, block, 0, st, src_key, src_idx, n, max_id,
                               d.shift, d.bits, cnt, totals, w.ntiles, dst_key, dst_idx);
        src_key = dst_key;
        src_idx = dst_idx;
    }
    hipLaunchKernelGGL(mg::group_seg_count_kernel, tiles, block, 0, st, src_key, n, segcnt);
    hipLaunchKernelGGL(mg::group_scan_kernel, dim3(1), block, 0, st, reinterpret_cast<uint4 *>(segcnt), w.ntiles,
                       segtot);
    hipLaunchKernelGGL(mg::group_seg_emit_kernel, tiles, block, 0, st, src_key, n, max_id, segcnt, segtot,
                       d_seg_sid, d_seg_start, d_nseg);
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

// m is known only on the device: a bounded call brings the whole piece down
// pinned and copies out what the contract names; an unbounded one fetches idx
// and nseg, waits, and fetches the table's m and m + 1 entries.
int mtcp_gpu_group(mtcp_gpu_ctx *ctx, const uint32_t *sid, uint32_t n, uint32_t max_id,
                   uint32_t *idx, uint32_t *seg_sid, uint32_t *seg_start, uint32_t *nseg) {
    if (!ctx || n > MTCP_GPU_GROUP_MAX_PKTS || max_id > MTCP_GPU_FLOWTAB_MAX_ID ||
        (n && (!sid || !idx || !seg_sid || !seg_start || !nseg)))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    const GroupLayout l(n, mg::group_work(n, max_id).bytes);
    Stage &s = ctx->stage[0];
    int rc = stage_reserve(ctx, s, l.dev_bytes, 0, dl);
    if (rc == MTCP_GPU_OK && dl.bounded) rc = stage_host(ctx, s, l.in_bytes, l.out_bytes(), dl);
    if (rc != MTCP_GPU_OK) return rc;
    Call hc(s, dl, {ctx, dl});
    hc.up(l.sid(s), sid, l.sid.bytes);
    if (hc.ok())
        hc.note(mtcp_gpu_group_dev(ctx, l.sid(s), n, max_id, l.idx(s), l.seg_sid(s), l.seg_start(s), l.nseg(s),
                                   l.work(s), l.work.bytes, s.stream));
    if (hc.bounded()) {
        // one wait: nothing has reached the caller when it gives up
        const uint8_t *h = hc.down_pinned(s.d_buf + l.back_off, l.back_bytes());
        if ((rc = hc.finish()) != MTCP_GPU_OK) return rc;
        l.copy_out(h, {{nseg, l.nseg}});
        const uint32_t m = nseg[0] = std::min(nseg[0], n);
        l.copy_out(h, {{idx, l.idx}, {seg_sid, l.seg_sid, (size_t)m * sizeof(uint32_t)},
                       {seg_start, l.seg_start, ((size_t)m + 1) * sizeof(uint32_t)}});
        return rc;
    }
    hc.down(idx, l.idx(s), l.idx.bytes);
    hc.down(nseg, l.nseg(s), l.nseg.bytes);
    if ((rc = hc.finish()) != MTCP_GPU_OK) return rc;
    const uint32_t m = std::min(nseg[0], n);
    hc.down(seg_sid, l.seg_sid(s), (size_t)m * sizeof(uint32_t));
    hc.down(seg_start, l.seg_start(s), ((size_t)m + 1) * sizeof(uint32_t));
    return hc.finish();
}

// ---- the per-stream receive walk -------------------------------
static_assert(sizeof(mtcp_gpu_rcv_state) == 64 && sizeof(mtcp_gpu_rcv_place) == 16, "mtcp_gpu_rcvwalk.h layouts");
static_assert(offsetof(mtcp_gpu_rcv_state, tcp_state) == 28 && offsetof(mtcp_gpu_rcv_state, frag) == 32 &&
              offsetof(mtcp_gpu_rcv_place, put_len) == 12 && offsetof(mtcp_gpu_rcv_place, verdict) == 14,
              "rcvwalk_kernels.hpp reads and writes the records as 16 B pieces");
static_assert(offsetof(mtcp_gpu_result, seq) == 12 && offsetof(mtcp_gpu_result, payload_len) == 32 &&
              offsetof(mtcp_gpu_result, tcp_flags) == 35, "rcvwalk_gather_kernel's two loads of a record");

uint32_t mtcp_gpu_rcvwalk_short_len(void) { return mg::kRcvShortLen; }

uint64_t mtcp_gpu_rcvwalk_work_bytes(uint32_t n, uint32_t max_id) {
    if (n > MTCP_GPU_GROUP_MAX_PKTS || max_id > MTCP_GPU_FLOWTAB_MAX_ID) return 0;
    return mg::rcv_work(n).bytes;
}

int mtcp_gpu_rcvwalk_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_result *d_res, const mtcp_gpu_tcpopt *d_opt,
                         uint32_t n, uint32_t max_id, const uint32_t *d_idx, const uint32_t *d_seg_sid,
                         const uint32_t *d_seg_start, const uint32_t *d_nseg, mtcp_gpu_rcv_state *d_state,
                         mtcp_gpu_rcv_place *d_place, uint32_t *d_seg_stop, void *d_work, uint64_t work_bytes,
                         void *stream) {
    if (!ctx || n > MTCP_GPU_GROUP_MAX_PKTS || max_id > MTCP_GPU_FLOWTAB_MAX_ID ||
        (ctx->flags & MTCP_GPU_F_COMPACT) ||
        (n && (!d_res || !d_idx || !d_seg_sid || !d_seg_start || !d_nseg || !d_state || !d_place || !d_seg_stop ||
               !d_work)) ||
        ((uintptr_t)d_res & 7) || ((uintptr_t)d_opt & 15) || ((uintptr_t)d_idx & 3) || ((uintptr_t)d_seg_sid & 3) ||
        ((uintptr_t)d_seg_start & 3) || ((uintptr_t)d_nseg & 3) || ((uintptr_t)d_state & 63) ||
        ((uintptr_t)d_place & 15) || ((uintptr_t)d_seg_stop & 3) || ((uintptr_t)d_work & 15))
        return MTCP_GPU_EINVAL;
    const mg::RcvWork w = mg::rcv_work(n);
    if (n && work_bytes < w.bytes) return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    hipStream_t st = pick(ctx, stream);
    const dim3 block(mg::kBlock), grid((n + mg::kBlock - 1) / mg::kBlock);
    uint4 *win = reinterpret_cast<uint4 *>(static_cast<uint8_t *>(d_work) + w.in_off);
    hipLaunchKernelGGL(mg::rcvwalk_gather_kernel, grid, block, 0, st, reinterpret_cast<const uint8_t *>(d_res),
                       reinterpret_cast<const uint4 *>(d_opt), d_idx, n, win, reinterpret_cast<uint4 *>(d_place));
    hipLaunchKernelGGL((mg::rcvwalk_walk_kernel<mg::kRcvShortLen, mg::kRcvWaveMax>), grid, block, 0, st, win, d_idx, n, max_id,
                       d_seg_sid, d_seg_start, d_nseg, d_opt ? 1u : 0u, reinterpret_cast<uint4 *>(d_state),
                       reinterpret_cast<uint4 *>(d_place), d_seg_stop);
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

// A bounded call brings the back piece (RcvwalkLayout) down pinned in one
// wait and copies out what the contract names: nothing has reached the caller
// when it gives up.
int mtcp_gpu_rcvwalk(mtcp_gpu_ctx *ctx, const mtcp_gpu_result *res, const mtcp_gpu_tcpopt *opt, uint32_t n,
                     uint32_t max_id, const uint32_t *idx, const uint32_t *seg_sid, const uint32_t *seg_start,
                     const uint32_t *nseg, mtcp_gpu_rcv_state *state, mtcp_gpu_rcv_place *place,
                     uint32_t *seg_stop) {
    if (!ctx || n > MTCP_GPU_GROUP_MAX_PKTS || max_id > MTCP_GPU_FLOWTAB_MAX_ID ||
        (ctx->flags & MTCP_GPU_F_COMPACT) ||
        (n && (!res || !idx || !seg_sid || !seg_start || !nseg || !state || !place || !seg_stop)))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    const uint32_t m = std::min(nseg[0], n);
    const RcvwalkLayout l(n, max_id, m, opt != nullptr, false, mg::rcv_work(n).bytes);
    Stage &s = ctx->stage[0];
    int rc = stage_reserve(ctx, s, l.dev_bytes, 0, dl);
    if (rc == MTCP_GPU_OK && dl.bounded) rc = stage_host(ctx, s, l.in_bytes, l.out_bytes(), dl);
    if (rc != MTCP_GPU_OK) return rc;
    Call hc(s, dl, {ctx, dl});
    hc.up(l.res(s), res, l.res.bytes);
    hc.up(l.opt(s), opt, l.opt.bytes);
    l.g.up(hc, s, idx, seg_sid, seg_start, &m);
    hc.up(l.state(s), state, l.state.bytes);
    if (hc.ok())
        hc.note(mtcp_gpu_rcvwalk_dev(ctx, l.res(s), opt ? l.opt(s) : nullptr, n, max_id, l.g.idx(s), l.g.seg_sid(s),
                                     l.g.seg_start(s), l.g.nseg(s), l.state(s), l.rec(s), l.stop(s), l.work(s),
                                     l.work.bytes, s.stream));
    const uint64_t mbytes = (uint64_t)m * sizeof(uint32_t);
    if (hc.bounded()) return l.fetch(hc, s, {{state, l.state}, {place, l.rec}, {seg_stop, l.stop, mbytes}});
    hc.down(state, l.state(s), l.state.bytes);
    hc.down(place, l.rec(s), l.rec.bytes);
    hc.down(seg_stop, l.stop(s), mbytes);
    return hc.finish();
}

// ---- the per-stream ProcessACK walk -----------------------------
static_assert(sizeof(mtcp_gpu_ack_state) == 128 && sizeof(mtcp_gpu_ack_rec) == 16, "mtcp_gpu_ackwalk.h layouts");
static_assert(offsetof(mtcp_gpu_ack_state, sb_head_seq) == 64 && offsetof(mtcp_gpu_ack_state, mss) == 76 &&
              offsetof(mtcp_gpu_ack_state, tcp_state) == 80 && offsetof(mtcp_gpu_ack_state, nrtx) == 84 &&
              offsetof(mtcp_gpu_ack_state, user) == 88 && offsetof(mtcp_gpu_ack_rec, flags) == 12 &&
              offsetof(mtcp_gpu_ack_rec, verdict) == 14,
              "ackwalk_kernels.hpp reads and writes the records as 16 B pieces");
static_assert(offsetof(mtcp_gpu_result, ack_seq) == 16 && offsetof(mtcp_gpu_result, window) == 20,
              "ackwalk_gather_kernel's loads of a record");

uint32_t mtcp_gpu_ackwalk_short_len(void) { return mg::kAckShortLen; }

uint64_t mtcp_gpu_ackwalk_work_bytes(uint32_t n, uint32_t max_id) {
    if (n > MTCP_GPU_GROUP_MAX_PKTS || max_id > MTCP_GPU_FLOWTAB_MAX_ID) return 0;
    return mg::ack_work(n).bytes;
}

int mtcp_gpu_ackwalk_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_result *d_res, const mtcp_gpu_tcpopt *d_opt,
                         const mtcp_gpu_rcv_place *d_place, uint32_t n, uint32_t max_id, const uint32_t *d_idx,
                         const uint32_t *d_seg_sid, const uint32_t *d_seg_start, const uint32_t *d_nseg,
                         uint32_t cur_ts, mtcp_gpu_ack_state *d_snd, mtcp_gpu_ack_rec *d_ack, uint32_t *d_ack_stop,
                         void *d_work, uint64_t work_bytes, void *stream) {
    if (!ctx || n > MTCP_GPU_GROUP_MAX_PKTS || max_id > MTCP_GPU_FLOWTAB_MAX_ID ||
        (ctx->flags & MTCP_GPU_F_COMPACT) ||
        (n && (!d_res || !d_place || !d_idx || !d_seg_sid || !d_seg_start || !d_nseg || !d_snd || !d_ack ||
               !d_ack_stop || !d_work)) ||
        ((uintptr_t)d_res & 7) || ((uintptr_t)d_opt & 15) || ((uintptr_t)d_place & 15) || ((uintptr_t)d_idx & 3) ||
        ((uintptr_t)d_seg_sid & 3) || ((uintptr_t)d_seg_start & 3) || ((uintptr_t)d_nseg & 3) ||
        ((uintptr_t)d_snd & 127) || ((uintptr_t)d_ack & 15) || ((uintptr_t)d_ack_stop & 3) || ((uintptr_t)d_work & 15))
        return MTCP_GPU_EINVAL;
    const mg::AckWork w = mg::ack_work(n);
    if (n && work_bytes < w.bytes) return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    hipStream_t st = pick(ctx, stream);
    const dim3 block(mg::kBlock), grid((n + mg::kBlock - 1) / mg::kBlock);
    uint4 *win = reinterpret_cast<uint4 *>(static_cast<uint8_t *>(d_work) + w.in_off);
    hipLaunchKernelGGL(mg::ackwalk_gather_kernel, grid, block, 0, st, reinterpret_cast<const uint8_t *>(d_res),
                       reinterpret_cast<const uint4 *>(d_opt), reinterpret_cast<const uint4 *>(d_place), d_idx, n, win,
                       reinterpret_cast<uint4 *>(d_ack));
    hipLaunchKernelGGL((mg::ackwalk_walk_kernel<mg::kAckShortLen, mg::kAckWaveMax>), grid, block, 0, st, win, d_idx, n, max_id,
                       d_seg_sid, d_seg_start, d_nseg, cur_ts, reinterpret_cast<uint4 *>(d_snd),
                       reinterpret_cast<uint4 *>(d_ack), d_ack_stop);
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

int mtcp_gpu_ackwalk(mtcp_gpu_ctx *ctx, const mtcp_gpu_result *res, const mtcp_gpu_tcpopt *opt,
                     const mtcp_gpu_rcv_place *place, uint32_t n, uint32_t max_id, const uint32_t *idx,
                     const uint32_t *seg_sid, const uint32_t *seg_start, const uint32_t *nseg, uint32_t cur_ts,
                     mtcp_gpu_ack_state *snd, mtcp_gpu_ack_rec *ack, uint32_t *ack_stop) {
    if (!ctx || n > MTCP_GPU_GROUP_MAX_PKTS || max_id > MTCP_GPU_FLOWTAB_MAX_ID ||
        (ctx->flags & MTCP_GPU_F_COMPACT) ||
        (n && (!res || !place || !idx || !seg_sid || !seg_start || !nseg || !snd || !ack || !ack_stop)))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    const uint32_t m = std::min(nseg[0], n);
    const AckwalkLayout l(n, max_id, m, opt != nullptr, true, mg::ack_work(n).bytes);
    Stage &s = ctx->stage[0];
    int rc = stage_reserve(ctx, s, l.dev_bytes, 0, dl);
    if (rc == MTCP_GPU_OK && dl.bounded) rc = stage_host(ctx, s, l.in_bytes, l.out_bytes(), dl);
    if (rc != MTCP_GPU_OK) return rc;
    Call hc(s, dl, {ctx, dl});
    hc.up(l.res(s), res, l.res.bytes);
    hc.up(l.opt(s), opt, l.opt.bytes);
    hc.up(l.place(s), place, l.place.bytes);
    l.g.up(hc, s, idx, seg_sid, seg_start, &m);
    hc.up(l.state(s), snd, l.state.bytes);
    if (hc.ok())
        hc.note(mtcp_gpu_ackwalk_dev(ctx, l.res(s), opt ? l.opt(s) : nullptr, l.place(s), n, max_id, l.g.idx(s),
                                     l.g.seg_sid(s), l.g.seg_start(s), l.g.nseg(s), cur_ts, l.state(s), l.rec(s),
                                     l.stop(s), l.work(s), l.work.bytes, s.stream));
    const uint64_t mbytes = (uint64_t)m * sizeof(uint32_t);
    if (hc.bounded()) return l.fetch(hc, s, {{snd, l.state}, {ack, l.rec}, {ack_stop, l.stop, mbytes}});
    hc.down(snd, l.state(s), l.state.bytes);
    hc.down(ack, l.rec(s), l.rec.bytes);
    hc.down(ack_stop, l.stop(s), mbytes);
    return hc.finish();
}

// ---- the payload copy behind the walk ---------------------------
static_assert(sizeof(mtcp_gpu_rcv_buf) == 32 && offsetof(mtcp_gpu_rcv_buf, size) == 8 &&
              offsetof(mtcp_gpu_rcv_buf, tail_offset) == 16 && offsetof(mtcp_gpu_rcv_buf, rsvd) == 24,
              "rcvcopy_plan_kernel reads and writes a record as two 16 B pieces");
static_assert(sizeof(mtcp_gpu_desc) == 8 && offsetof(mtcp_gpu_desc, len) == 4 &&
              offsetof(mtcp_gpu_result, ihl_doff) == 34, "rcvcopy_prep_kernel's loads");

uint64_t mtcp_gpu_rcvcopy_work_bytes(uint32_t n, uint32_t max_id) {
    if (n > MTCP_GPU_GROUP_MAX_PKTS || max_id > MTCP_GPU_FLOWTAB_MAX_ID) return 0;
    return mg::copy_work(n).bytes;
}

int mtcp_gpu_rcvcopy_dev(mtcp_gpu_ctx *ctx, const void *d_buf, uint64_t buf_len, const mtcp_gpu_desc *d_desc,
                         uint32_t off_shift, const mtcp_gpu_result *d_res, const mtcp_gpu_rcv_place *d_place,
                         uint32_t n, uint32_t max_id, const uint32_t *d_idx, const uint32_t *d_seg_sid,
                         const uint32_t *d_seg_start, const uint32_t *d_nseg, const uint32_t *d_seg_stop,
                         mtcp_gpu_rcv_buf *d_rbuf, void *d_arena, uint64_t arena_bytes, uint8_t *d_cstat,
                         void *d_work, uint64_t work_bytes, void *stream) {
    if (!ctx || n > MTCP_GPU_GROUP_MAX_PKTS || max_id > MTCP_GPU_FLOWTAB_MAX_ID ||
        (ctx->flags & MTCP_GPU_F_COMPACT) || off_shift > 16 || (buf_len & 15) ||
        (n && (!d_buf || !d_desc || !d_res || !d_place || !d_idx || !d_seg_sid || !d_seg_start || !d_nseg ||
               !d_seg_stop || !d_rbuf || !d_arena || !d_cstat || !d_work)) ||
        ((uintptr_t)d_buf & 15) || ((uintptr_t)d_desc & 7) || ((uintptr_t)d_res & 7) || ((uintptr_t)d_place & 15) ||
        ((uintptr_t)d_idx & 3) || ((uintptr_t)d_seg_sid & 3) || ((uintptr_t)d_seg_start & 3) ||
        ((uintptr_t)d_nseg & 3) || ((uintptr_t)d_seg_stop & 3) || ((uintptr_t)d_rbuf & 31) ||
        ((uintptr_t)d_arena & 15) || ((uintptr_t)d_work & 15))
        return MTCP_GPU_EINVAL;
    const mg::CopyWork w = mg::copy_work(n);
    if (n && work_bytes < w.bytes) return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    hipStream_t st = pick(ctx, stream);
    const dim3 block(mg::kBlock), grid((n + mg::kBlock - 1) / mg::kBlock);
    uint8_t *work = static_cast<uint8_t *>(d_work);
    uint4 *win = reinterpret_cast<uint4 *>(work + w.in_off), *wsum = reinterpret_cast<uint4 *>(work + w.sum_off);
    uint2 *wplan = reinterpret_cast<uint2 *>(work + w.plan_off);
    const uint64_t buf = reinterpret_cast<uint64_t>(d_buf), arena = reinterpret_cast<uint64_t>(d_arena);
    hipLaunchKernelGGL(mg::rcvcopy_prep_kernel, grid, block, 0, st, reinterpret_cast<const uint8_t *>(d_res),
                       reinterpret_cast<const uint4 *>(d_place), reinterpret_cast<const uint2 *>(d_desc), off_shift,
                       buf_len, d_idx, n, win, wplan, d_cstat);
    hipLaunchKernelGGL(mg::rcvcopy_plan_kernel, grid, block, 0, st, win, d_idx, n, max_id, d_seg_sid, d_seg_start,
                       d_nseg, d_seg_stop, reinterpret_cast<uint4 *>(d_rbuf), arena, arena_bytes, wplan, wsum, d_cstat);
    const int group = rcvcopy_group(buf_len, n);
    const dim3 fgrid((uint32_t)(((uint64_t)n * group + mg::kBlock - 1) / mg::kBlock));
    if (group == 8)
        hipLaunchKernelGGL(mg::rcvcopy_front_kernel<8>, fgrid, block, 0, st, buf, win, wplan, wsum, n, arena);
    else
        hipLaunchKernelGGL(mg::rcvcopy_front_kernel<32>, fgrid, block, 0, st, buf, win, wplan, wsum, n, arena);
    hipLaunchKernelGGL(mg::rcvcopy_ordered_kernel, grid, block, 0, st, buf, win, wplan, wsum, n, max_id, d_seg_sid,
                       d_seg_start, d_nseg, d_seg_stop, arena);
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

// ---- device flow table ----------------------------------------
}  // extern "C"

// The mirror of one tcp_flow_table (fhash.c:16-56).  Bound to its context:
// it is created, destroyed and used through that context's device, stream and
// wait limit.
struct mtcp_gpu_flowtab {
    mtcp_gpu_ctx *ctx = nullptr;
    uint32_t cap_log2 = 0;
    uint4 *slots = nullptr;              // 2^cap_log2 of them (park.hpp)
    uint32_t *stats = nullptr;           // mtcp_gpu_flowtab_counters on the device
    mtcp_gpu_flowtab_counters *h_stats = nullptr;   // pinned, for the bounded stats call
};

namespace {

static_assert(sizeof(mtcp_gpu_flow_entry) == 16 && sizeof(mtcp_gpu_flowtab_counters) == 16,
              "mtcp_gpu_flowtab.h layouts");
static_assert(MTCP_GPU_FLOWTAB_MIN_CAP_LOG2 >= 2, "flowtab_lookup_kernel<4> walks the slots four at a time");

// slots loaded per probe step of the lookup (flowtab_kernels.hpp)
constexpr int kFlowtabGroup = 4;

size_t flowtab_bytes(const mtcp_gpu_flowtab *t) { return sizeof(uint4) << t->cap_log2; }
uint32_t flowtab_mask(const mtcp_gpu_flowtab *t) { return (1u << t->cap_log2) - 1; }

// one lane per entry or slot, up to 8 workgroups per CU, grid-stride beyond
dim3 flowtab_grid(const mtcp_gpu_ctx *ctx, uint32_t n) {
    return dim3(std::max(1u, std::min<uint32_t>((n + mg::kBlock - 1) / mg::kBlock, (uint32_t)ctx->num_cu * 8)));
}

bool flowtab_ids_ok(const mtcp_gpu_flow_entry *e, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i)
        if (e[i].id > MTCP_GPU_FLOWTAB_MAX_ID) return false;
    return true;
}

}  // namespace

extern "C" {

uint32_t mtcp_gpu_flowtab_home(const void *key12, uint32_t cap_log2) {
    if (!key12 || cap_log2 < MTCP_GPU_FLOWTAB_MIN_CAP_LOG2 || cap_log2 > MTCP_GPU_FLOWTAB_MAX_CAP_LOG2)
        return 0xFFFFFFFFu;
    uint32_t key[3];
    memcpy(key, key12, 12);
    return mg::flowtab_home(key, (1u << cap_log2) - 1);
}

int mtcp_gpu_flowtab_create(mtcp_gpu_ctx *ctx, uint32_t cap_log2, mtcp_gpu_flowtab **tab) {
    if (tab) *tab = nullptr;
    if (!ctx || !tab || cap_log2 < MTCP_GPU_FLOWTAB_MIN_CAP_LOG2 || cap_log2 > MTCP_GPU_FLOWTAB_MAX_CAP_LOG2)
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    DeviceGuard dg(ctx->device);
    if (!dg.ok) return MTCP_GPU_ENODEV;
    mtcp_gpu_flowtab *t = new (std::nothrow) mtcp_gpu_flowtab;
    if (!t) return MTCP_GPU_ENOMEM;
    t->ctx = ctx;
    t->cap_log2 = cap_log2;
    const Deadline dl(ctx->wait_us);
    int rc = MTCP_GPU_OK;
    if (!HIP_OK(mtcp_park::alloc(&t->slots, flowtab_bytes(t), mtcp_park::kDevice)) ||
        !HIP_OK(mtcp_park::alloc(&t->stats, 16, mtcp_park::kDevice)) ||
        !HIP_OK(mtcp_park::alloc(&t->h_stats, 16, mtcp_park::kHost)))
        rc = MTCP_GPU_ENOMEM;
    // every slot EMPTY (all bytes 0xFF), every counter 0
    if (rc == MTCP_GPU_OK && (!HIP_OK(hipMemsetAsync(t->slots, 0xFF, flowtab_bytes(t), ctx->stream)) ||
                              !HIP_OK(hipMemsetAsync(t->stats, 0, 16, ctx->stream))))
        rc = MTCP_GPU_EIO;
    if (rc == MTCP_GPU_OK) rc = waited(ctx, drain(ctx->stream, dl));
    if (rc != MTCP_GPU_OK) {
        if (rc != MTCP_GPU_ETIMEDOUT) {          // past the limit the clears may still run: the buffers stay
            mtcp_park::release(t->slots, flowtab_bytes(t), mtcp_park::kDevice, !dl.bounded);
            mtcp_park::release(t->stats, 16, mtcp_park::kDevice, !dl.bounded);
            mtcp_park::release(t->h_stats, 16, mtcp_park::kHost, !dl.bounded);
        }
        delete t;
        return rc;
    }
    *tab = t;
    return MTCP_GPU_OK;
}

void mtcp_gpu_flowtab_destroy(mtcp_gpu_flowtab *tab) {
    if (!tab) return;
    if (!tab->ctx->abandoned) {                  // abandoned: work given up on may still use the buffers
        DeviceGuard dg(tab->ctx->device);
        const bool may_free = tab->ctx->wait_us == 0;
        mtcp_park::release(tab->slots, flowtab_bytes(tab), mtcp_park::kDevice, may_free);
        mtcp_park::release(tab->stats, 16, mtcp_park::kDevice, may_free);
        mtcp_park::release(tab->h_stats, 16, mtcp_park::kHost, may_free);
    }
    delete tab;
}

uint32_t mtcp_gpu_flowtab_capacity(const mtcp_gpu_flowtab *tab) { return tab ? 1u << tab->cap_log2 : 0u; }

int mtcp_gpu_flowtab_update_dev(mtcp_gpu_flowtab *tab, const mtcp_gpu_flow_entry *d_del, uint32_t n_del,
                                const mtcp_gpu_flow_entry *d_ins, uint32_t n_ins, void *stream) {
    if (!tab || (n_del && !d_del) || (n_ins && !d_ins) || ((uintptr_t)d_del & 15) || ((uintptr_t)d_ins & 15) ||
        n_del > MTCP_GPU_FLOWTAB_MAX_BATCH || n_ins > MTCP_GPU_FLOWTAB_MAX_BATCH)
        return MTCP_GPU_EINVAL;
    mtcp_gpu_ctx *ctx = tab->ctx;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n_del == 0 && n_ins == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    hipStream_t st = pick(ctx, stream);
    if (n_del)
        hipLaunchKernelGGL(mg::flowtab_remove_kernel, flowtab_grid(ctx, n_del), dim3(mg::kBlock), 0, st, tab->slots,
                           flowtab_mask(tab), reinterpret_cast<const uint4 *>(d_del), n_del, tab->stats);
    if (n_ins)
        hipLaunchKernelGGL(mg::flowtab_insert_kernel, flowtab_grid(ctx, n_ins), dim3(mg::kBlock), 0, st, tab->slots,
                           flowtab_mask(tab), reinterpret_cast<const uint4 *>(d_ins), n_ins, tab->stats);
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

int mtcp_gpu_flowtab_lookup_dev(mtcp_gpu_flowtab *tab, const mtcp_gpu_result *d_res, uint32_t n,
                                uint32_t *d_sid, uint32_t *d_bins, void *stream) {
    if (!tab || (n && (!d_res || !d_sid)) || ((uintptr_t)d_res & 7) || ((uintptr_t)d_sid & 3) ||
        ((uintptr_t)d_bins & 3) || n > MTCP_GPU_FLOWTAB_MAX_BATCH ||
        (tab->ctx->flags & MTCP_GPU_F_COMPACT))     // reads 40 B records (the 4-tuple)
        return MTCP_GPU_EINVAL;
    mtcp_gpu_ctx *ctx = tab->ctx;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    hipLaunchKernelGGL(mg::flowtab_lookup_kernel<kFlowtabGroup>, flowtab_grid(ctx, n), dim3(mg::kBlock), 0,
                       pick(ctx, stream), d_res, n, tab->slots, flowtab_mask(tab), d_sid, d_bins);
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

// The entries go up into stage 0's chunk buffer (removes, then inserts,
// adjacent: they go up together), the kernels run behind them.
int mtcp_gpu_flowtab_update(mtcp_gpu_flowtab *tab, const mtcp_gpu_flow_entry *del, uint32_t n_del,
                            const mtcp_gpu_flow_entry *ins, uint32_t n_ins) {
    if (!tab || (n_del && !del) || (n_ins && !ins) || n_del > MTCP_GPU_FLOWTAB_MAX_BATCH ||
        n_ins > MTCP_GPU_FLOWTAB_MAX_BATCH || !flowtab_ids_ok(del, n_del) || !flowtab_ids_ok(ins, n_ins))
        return MTCP_GPU_EINVAL;
    mtcp_gpu_ctx *ctx = tab->ctx;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n_del == 0 && n_ins == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    const uint64_t dbytes = (uint64_t)n_del * 16, ibytes = (uint64_t)n_ins * 16;
    Stage &s = ctx->stage[0];
    int rc = stage_reserve(ctx, s, dbytes + ibytes, 0, dl);
    if (rc == MTCP_GPU_OK && dl.bounded) rc = stage_host(ctx, s, dbytes + ibytes, 0, dl);
    if (rc != MTCP_GPU_OK) return rc;
    const mtcp_gpu_flow_entry *d_del = reinterpret_cast<const mtcp_gpu_flow_entry *>(s.d_buf);
    const mtcp_gpu_flow_entry *d_ins = d_del + n_del;
    Call hc(s, dl, {ctx, dl});
    hc.up2(s.d_buf, del, dbytes, ins, ibytes);
    if (hc.ok())
        hc.note(mtcp_gpu_flowtab_update_dev(tab, n_del ? d_del : nullptr, n_del, n_ins ? d_ins : nullptr, n_ins,
                                            s.stream));
    return hc.finish();
}

// The records go up into stage 0's record buffer; its chunk buffer holds
// sid[n], then bins[n] (adjacent: they come down together).
int mtcp_gpu_flowtab_lookup(mtcp_gpu_flowtab *tab, const mtcp_gpu_result *res, uint32_t n, uint32_t *sid,
                            uint32_t *bins) {
    if (!tab || (n && (!res || !sid)) || n > MTCP_GPU_FLOWTAB_MAX_BATCH || (tab->ctx->flags & MTCP_GPU_F_COMPACT))
        return MTCP_GPU_EINVAL;
    mtcp_gpu_ctx *ctx = tab->ctx;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    const uint64_t rbytes = (uint64_t)n * sizeof(mtcp_gpu_result), sbytes = (uint64_t)n * sizeof(uint32_t);
    const uint64_t obytes = bins ? 2 * sbytes : sbytes;
    Stage &s = ctx->stage[0];
    int rc = stage_reserve(ctx, s, obytes, n, dl);
    if (rc == MTCP_GPU_OK && dl.bounded) rc = stage_host(ctx, s, rbytes, obytes, dl);
    if (rc != MTCP_GPU_OK) return rc;
    uint32_t *d_sid = reinterpret_cast<uint32_t *>(s.d_buf);
    uint32_t *d_bins = bins ? d_sid + n : nullptr;
    Call hc(s, dl, {ctx, dl});
    hc.up(s.d_out, res, rbytes);
    if (hc.ok()) hc.note(mtcp_gpu_flowtab_lookup_dev(tab, s.d_out, n, d_sid, d_bins, s.stream));
    hc.down2(sid, d_sid, sbytes, bins, bins ? sbytes : 0);
    return hc.finish();
}

int mtcp_gpu_flowtab_stats(mtcp_gpu_flowtab *tab, mtcp_gpu_flowtab_counters *stats) {
    if (!tab || !stats) return MTCP_GPU_EINVAL;
    mtcp_gpu_ctx *ctx = tab->ctx;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    int rc = HIP_OK(hipMemcpyAsync(tab->h_stats, tab->stats, 16, hipMemcpyDeviceToHost, ctx->stream))
                 ? waited(ctx, drain(ctx->stream, dl)) : MTCP_GPU_EIO;
    if (rc == MTCP_GPU_OK) *stats = *tab->h_stats;
    return rc;
}

int mtcp_gpu_flowtab_rehash(mtcp_gpu_flowtab *tab) {
    if (!tab) return MTCP_GPU_EINVAL;
    mtcp_gpu_ctx *ctx = tab->ctx;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    uint4 *fresh = nullptr;
    if (!HIP_OK(mtcp_park::alloc(&fresh, flowtab_bytes(tab), mtcp_park::kDevice))) return MTCP_GPU_ENOMEM;
    int rc = MTCP_GPU_OK;
    // live and tombs (the first 8 B of the counters) start again from 0
    if (!HIP_OK(hipMemsetAsync(fresh, 0xFF, flowtab_bytes(tab), ctx->stream)) ||
        !HIP_OK(hipMemsetAsync(tab->stats, 0, 8, ctx->stream)))
        rc = MTCP_GPU_EIO;
    if (rc == MTCP_GPU_OK) {
        hipLaunchKernelGGL(mg::flowtab_rehash_kernel, flowtab_grid(ctx, 1u << tab->cap_log2), dim3(mg::kBlock), 0,
                           ctx->stream, tab->slots, fresh, flowtab_mask(tab), tab->stats);
        if (!HIP_OK(hipGetLastError())) rc = MTCP_GPU_EIO;
    }
    rc = waited(ctx, rc == MTCP_GPU_OK ? drain(ctx->stream, dl) : rc);
    if (rc == MTCP_GPU_ETIMEDOUT) return rc;     // both arrays stay: the launch may still run
    if (rc == MTCP_GPU_OK) std::swap(fresh, tab->slots);
    mtcp_park::release(fresh, flowtab_bytes(tab), mtcp_park::kDevice, !dl.bounded);
    return rc;
}

// ---- tx frames from segment records --------------------------
namespace {

static_assert(sizeof(mtcp_gpu_tx_seg) == 48 && sizeof(mtcp_gpu_tx_link) == 12, "mtcp_gpu_txbuild.h layouts");

bool txbuild_args_ok(const mtcp_gpu_ctx *ctx, uint32_t n, const void *seg, const void *payload,
                     uint64_t payload_bytes, const void *links, uint32_t n_links, const void *buf,
                     uint64_t buf_len, const void *desc, uint32_t off_shift, uint32_t flags, const void *status) {
    if (!ctx || (flags & ~MTCP_GPU_TXB_NO_CSUM) || off_shift > 16 || n_links < 1 ||
        n_links > MTCP_GPU_TXB_MAX_LINKS)
        return false;
    if (n && (!seg || !links || !buf || !desc || !status || (!payload && payload_bytes))) return false;
    // the builder reads the payload while it writes frames: the two ranges are apart
    const uintptr_t p0 = (uintptr_t)payload, b0 = (uintptr_t)buf;
    if (n && payload_bytes && buf_len && p0 < b0 + buf_len && b0 < p0 + payload_bytes) return false;
    return true;
}

// The built frames' bytes from the image in pinned staging into the caller's
// buf; returns their number.
static uint32_t copy_built(void *buf, const uint8_t *image, uint64_t buf_len, const mtcp_gpu_desc *desc,
                    const uint8_t *status, uint32_t n, uint32_t off_shift) {
    uint32_t cnt = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t off = (uint64_t)desc[i].offset << off_shift;
        // the kernel builds only frames inside the image (checked again here)
        if (status[i] != MTCP_GPU_TXB_BUILT || off > buf_len || desc[i].len > buf_len - off) continue;
        memcpy(static_cast<uint8_t *>(buf) + off, image + off, desc[i].len);
        ++cnt;
    }
    return cnt;
}

// A staging capacity for `need`: the next power of two once the present one
// is too small (a context grows O(log n) times, not once per new
// maximum).
uint64_t grown(uint64_t need, uint64_t have) {
    if (need <= have) return need;
    uint64_t cap = 4096;
    while (cap < need) cap <<= 1;
    return cap;
}

// Stage s for a call laid out by l that brings its results down pinned in
// either mode, behind first_bytes of its own (a tx call's image).
int stage_pinned(mtcp_gpu_ctx *ctx, Stage &s, const StageLayout &l, uint64_t first_bytes, uint32_t pkts,
                 const Deadline &dl) {
    const int rc = stage_reserve(ctx, s, grown(l.dev_bytes, s.buf_cap), pkts, dl);
    if (rc != MTCP_GPU_OK) return rc;
    return stage_host(ctx, s, dl.bounded ? grown(l.in_bytes, s.h_in_cap) : 0,
                      grown(l.out_bytes(first_bytes), s.h_out_cap), dl);
}

}  // namespace

int mtcp_gpu_tx_build_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_tx_seg *d_seg, uint32_t n,
                          const void *d_payload, uint64_t payload_bytes,
                          const mtcp_gpu_tx_link *d_links, uint32_t n_links,
                          void *d_buf, uint64_t buf_len, const mtcp_gpu_desc *d_desc, uint32_t off_shift,
                          uint16_t max_mss, uint32_t flags, uint8_t *d_status, void *stream) {
    if (!txbuild_args_ok(ctx, n, d_seg, d_payload, payload_bytes, d_links, n_links, d_buf, buf_len, d_desc,
                         off_shift, flags, d_status) ||
        ((uintptr_t)d_seg & 7) || ((uintptr_t)d_desc & 7) || ((uintptr_t)d_links & 3))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    mg::TxBuildParams p{};
    p.seg = d_seg;
    p.payload = static_cast<const uint8_t *>(d_payload);
    p.payload_bytes = payload_bytes;
    p.links = d_links;
    p.n_links = n_links;
    p.n = n;
    p.buf = static_cast<uint8_t *>(d_buf);
    p.buf_len = buf_len;
    p.desc = d_desc;
    p.off_shift = off_shift;
    p.max_mss = max_mss ? max_mss : MTCP_GPU_TXB_DEFAULT_MSS;
    p.no_csum = flags & MTCP_GPU_TXB_NO_CSUM;
    p.status = d_status;
    const int group = txbuild_group(payload_bytes, n);
    const uint32_t per_block = mg::kBlock / group;
    const dim3 grid(std::min<uint32_t>((n + per_block - 1) / per_block, (uint32_t)ctx->num_cu * 8));
    hipStream_t st = pick(ctx, stream);
    if (group == 64)
        hipLaunchKernelGGL(mg::txbuild_kernel<64>, grid, dim3(mg::kBlock), 0, st, p);
    else if (group == 32)
        hipLaunchKernelGGL(mg::txbuild_kernel<32>, grid, dim3(mg::kBlock), 0, st, p);
    else if (group == 16)
        hipLaunchKernelGGL(mg::txbuild_kernel<16>, grid, dim3(mg::kBlock), 0, st, p);
    else
        hipLaunchKernelGGL(mg::txbuild_kernel<8>, grid, dim3(mg::kBlock), 0, st, p);
    ctx->last_kernel = group == 64   ? "txbuild_kernel<wave>"
                       : group == 32 ? "txbuild_kernel<half>"
                       : group == 16 ? "txbuild_kernel<row>" : "txbuild_kernel<oct>";
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

// The image is never uploaded (the builder reads no frame byte) and comes
// down pinned, whole, with the status bytes behind it, from where only the
// built frames' bytes reach buf.
int mtcp_gpu_tx_build(mtcp_gpu_ctx *ctx, const mtcp_gpu_tx_seg *seg, uint32_t n,
                      const void *payload, uint64_t payload_bytes,
                      const mtcp_gpu_tx_link *links, uint32_t n_links,
                      void *buf, uint64_t buf_len, const mtcp_gpu_desc *desc, uint32_t off_shift,
                      uint16_t max_mss, uint32_t flags, uint8_t *status, uint32_t *n_built) {
    if (!txbuild_args_ok(ctx, n, seg, payload, payload_bytes, links, n_links, buf, buf_len, desc, off_shift,
                         flags, status))
        return MTCP_GPU_EINVAL;
    if (n_built) *n_built = 0;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    Stage &s = ctx->stage[0];
    const TxLayout l(n, n_links, payload_bytes, buf_len);
    int rc = stage_pinned(ctx, s, l, buf_len, (uint32_t)grown(n, s.pkt_cap), dl);
    if (rc != MTCP_GPU_OK) return rc;
    Call hc(s, dl, {ctx, dl});
    hc.up(l.payload(s), payload, payload_bytes, true);
    hc.up(l.seg(s), seg, l.seg.bytes);
    hc.up(l.links(s), links, l.links.bytes);
    hc.up(s.d_desc, desc, (uint64_t)n * sizeof(mtcp_gpu_desc));
    if (hc.ok())
        hc.note(mtcp_gpu_tx_build_dev(ctx, l.seg(s), n, l.payload(s), payload_bytes, l.links(s), n_links, l.image(s),
                                      buf_len, s.d_desc, off_shift, max_mss, flags, l.status(s), s.stream));
    const uint8_t *image = hc.down_pinned(l.image(s), buf_len);
    if ((rc = l.fetch(hc, s, {{status, l.status}})) != MTCP_GPU_OK) return rc;
    const uint32_t cnt = copy_built(buf, image, buf_len, desc, status, n, off_shift);
    if (n_built) *n_built = cnt;
    return MTCP_GPU_OK;
}

// ---- tx segments from send bursts ----------------------------
namespace {

static_assert(sizeof(mtcp_gpu_tx_burst) == 64 && sizeof(mtcp_gpu_tx_burst_result) == 16, "mtcp_gpu_txseg.h layouts");
static_assert(mg::kTxsegOneSegs <= MTCP_GPU_TXSEG_MAX_SEGS, "the one-workgroup form is a seg_cap the ABI allows");

// What the host plan and the device calls refuse alike.
bool txseg_geom_ok(uint32_t n_burst, uint32_t n_links, uint64_t buf_off, uint32_t off_shift, uint32_t slot_bytes,
                   uint32_t seg_cap) {
    if (off_shift > 16 || n_links < 1 || n_links > MTCP_GPU_TXB_MAX_LINKS || seg_cap == 0 ||
        seg_cap > MTCP_GPU_TXSEG_MAX_SEGS || n_burst > MTCP_GPU_TXSEG_MAX_BURSTS)
        return false;
    const uint64_t A = off_shift ? 1ull << off_shift : 2ull;
    return (slot_bytes & (A - 1)) == 0 && (buf_off & (A - 1)) == 0;
}

// The workspace: the parked plans (16 B each), first[n] (u32), boff[n] (u64),
// the plan workgroups' sums (u32 and u64 each) and the totals, each part 16 B
// aligned.
struct TxSegWork {
    uint32_t nwg;
    uint64_t first_off, boff_off, pc_off, pb_off, tot_off, bytes;
};
TxSegWork txseg_work(uint32_t n) {
    TxSegWork w{};
    w.nwg = (n + mg::kTxsegTile - 1) / mg::kTxsegTile;
    w.first_off = 16ull * n;
    w.boff_off = w.first_off + pad16(4ull * n);
    w.pc_off = w.boff_off + pad16(8ull * n);
    w.pb_off = w.pc_off + pad16(4ull * w.nwg);
    w.tot_off = w.pb_off + pad16(8ull * w.nwg);
    w.bytes = w.tot_off + 16;
    return w;
}

bool txseg_dev_args_ok(const mtcp_gpu_ctx *ctx, const void *d_burst, uint32_t n_burst, uint32_t n_links,
                       uint64_t buf_off, uint32_t off_shift, uint32_t slot_bytes, const void *d_seg,
                       const void *d_desc, uint32_t seg_cap, const void *d_res, const void *d_total,
                       const void *d_work, uint64_t work_bytes) {
    if (!ctx || !txseg_geom_ok(n_burst, n_links, buf_off, off_shift, slot_bytes, seg_cap)) return false;
    if (!d_seg || !d_desc || !d_total || !d_work || (n_burst && (!d_burst || !d_res))) return false;
    if (((uintptr_t)d_burst & 7) || ((uintptr_t)d_seg & 7) || ((uintptr_t)d_desc & 7) || ((uintptr_t)d_res & 7) ||
        ((uintptr_t)d_total & 7) || ((uintptr_t)d_work & 15))
        return false;
    return work_bytes >= txseg_work(n_burst).bytes;
}

}  // namespace

int mtcp_gpu_tx_segment_plan(const mtcp_gpu_tx_burst *burst, uint32_t n_burst, uint64_t payload_bytes,
                             uint32_t n_links, uint64_t buf_off, uint64_t buf_len, uint32_t off_shift,
                             uint32_t slot_bytes, uint32_t seg_cap, uint16_t max_mss,
                             mtcp_gpu_tx_burst_result *res, uint64_t total[2]) {
    if (!txseg_geom_ok(n_burst, n_links, buf_off, off_shift, slot_bytes, seg_cap) || !total ||
        (n_burst && (!burst || !res)))
        return MTCP_GPU_EINVAL;
    const mg::TxSegParams P =
        mg::txseg_params(payload_bytes, n_links, buf_off, buf_len, off_shift, slot_bytes, seg_cap, max_mss);
    uint32_t S = 0, T = 0;             // the planned prefix (saturating, as on the device), the emitted total
    uint64_t B = 0, used = 0;
    bool cut = false;
    for (uint32_t i = 0; i < n_burst; ++i) {
        uint32_t w[16];
        memcpy(w, &burst[i], sizeof w);
        const mg::TxPlan pl = mg::txseg_plan(mg::txseg_unpack(w), P);
        const mg::TxEmit em = mg::txseg_emitted(pl, S, B, P);
        uint32_t r[4];
        mg::txseg_result(pl, em, cut ? T : S, r);
        memcpy(&res[i], r, sizeof r);
        if (!cut) {
            T = S + em.n;
            used = B + em.slot_sum;
            cut = em.n < pl.count;
        }
        S = mg::txseg_add_c(S, pl.count < seg_cap ? pl.count : seg_cap, seg_cap);
        B = mg::txseg_add_b(B, pl.slot_sum);
    }
    total[0] = T;
    total[1] = used;
    return MTCP_GPU_OK;
}

uint32_t mtcp_gpu_tx_segment_tile(void) { return mg::kTxsegTile; }

uint64_t mtcp_gpu_tx_segment_work_bytes(uint32_t n_burst) {
    return n_burst > MTCP_GPU_TXSEG_MAX_BURSTS ? 0 : txseg_work(n_burst).bytes;
}

int mtcp_gpu_tx_segment_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_tx_burst *d_burst, uint32_t n_burst,
                            uint64_t payload_bytes, uint32_t n_links, uint64_t buf_off, uint64_t buf_len,
                            uint32_t off_shift, uint32_t slot_bytes, uint16_t max_mss,
                            mtcp_gpu_tx_seg *d_seg, mtcp_gpu_desc *d_desc, uint32_t seg_cap,
                            mtcp_gpu_tx_burst_result *d_res, uint64_t *d_total,
                            void *d_work, uint64_t work_bytes, void *stream) {
    if (!txseg_dev_args_ok(ctx, d_burst, n_burst, n_links, buf_off, off_shift, slot_bytes, d_seg, d_desc, seg_cap,
                           d_res, d_total, d_work, work_bytes))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    DeviceGuard dg(ctx->device);
    hipStream_t st = pick(ctx, stream);
    const mg::TxSegParams P =
        mg::txseg_params(payload_bytes, n_links, buf_off, buf_len, off_shift, slot_bytes, seg_cap, max_mss);
    const dim3 block(mg::kBlock);
    if (n_burst <= mg::kTxsegTile && seg_cap <= mg::kTxsegOneSegs) {
        hipLaunchKernelGGL(mg::txseg_one_kernel, dim3(1), dim3(mg::kTxsegOneBlock), 0, st, d_burst, n_burst, P, d_seg, d_desc, d_res,
                           d_total);
        ctx->last_kernel = "txseg_one_kernel";
        return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
    }
    const TxSegWork w = txseg_work(n_burst);
    uint8_t *work = static_cast<uint8_t *>(d_work);
    mg::v4u *park = reinterpret_cast<mg::v4u *>(work);
    uint32_t *first = reinterpret_cast<uint32_t *>(work + w.first_off);
    uint64_t *boff = reinterpret_cast<uint64_t *>(work + w.boff_off);
    uint32_t *part_c = reinterpret_cast<uint32_t *>(work + w.pc_off);
    uint64_t *part_b = reinterpret_cast<uint64_t *>(work + w.pb_off);
    unsigned long long *tot_b = reinterpret_cast<unsigned long long *>(work + w.tot_off);
    uint32_t *tot_c = reinterpret_cast<uint32_t *>(work + w.tot_off + 8);
    if (n_burst) {
        hipLaunchKernelGGL(mg::txseg_plan_kernel, dim3(w.nwg), block, 0, st, d_burst, n_burst, P, park, part_c,
                           part_b);
        hipLaunchKernelGGL(mg::txseg_scan_kernel, dim3(1), block, 0, st, part_c, part_b, w.nwg, seg_cap, tot_c,
                           tot_b);
        hipLaunchKernelGGL(mg::txseg_place_kernel, dim3(w.nwg), block, 0, st, park, n_burst, P, part_c, part_b,
                           first, boff, d_res, tot_c, tot_b);
    }
    const uint32_t etiles = (seg_cap + mg::kTxsegEmitTile - 1) / mg::kTxsegEmitTile;
    hipLaunchKernelGGL(mg::txseg_emit_kernel, dim3(etiles), block, 0, st, d_burst, n_burst, P, first, boff, tot_c,
                       tot_b, d_seg, d_desc, d_res, d_total);
    ctx->last_kernel = "txseg_emit_kernel";
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

int mtcp_gpu_tx_send_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_tx_burst *d_burst, uint32_t n_burst,
                         const void *d_payload, uint64_t payload_bytes,
                         const mtcp_gpu_tx_link *d_links, uint32_t n_links,
                         void *d_buf, uint64_t buf_off, uint64_t buf_len, uint32_t off_shift,
                         uint32_t slot_bytes, uint16_t max_mss, uint32_t flags,
                         mtcp_gpu_tx_seg *d_seg, mtcp_gpu_desc *d_desc, uint32_t seg_cap,
                         mtcp_gpu_tx_burst_result *d_res, uint64_t *d_total, uint8_t *d_status,
                         void *d_work, uint64_t work_bytes, void *stream) {
    // both calls' checks before either launches
    if (!txseg_dev_args_ok(ctx, d_burst, n_burst, n_links, buf_off, off_shift, slot_bytes, d_seg, d_desc, seg_cap,
                           d_res, d_total, d_work, work_bytes) ||
        !txbuild_args_ok(ctx, seg_cap, d_seg, d_payload, payload_bytes, d_links, n_links, d_buf, buf_len, d_desc,
                         off_shift, flags, d_status) ||
        ((uintptr_t)d_links & 3))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    const int rc = mtcp_gpu_tx_segment_dev(ctx, d_burst, n_burst, payload_bytes, n_links, buf_off, buf_len, off_shift,
                                           slot_bytes, max_mss, d_seg, d_desc, seg_cap, d_res, d_total, d_work,
                                           work_bytes, stream);
    if (rc != MTCP_GPU_OK) return rc;
    return mtcp_gpu_tx_build_dev(ctx, d_seg, seg_cap, d_payload, payload_bytes, d_links, n_links, d_buf, buf_len,
                                 d_desc, off_shift, max_mss, flags, d_status, stream);
}

// The image is never uploaded and comes down pinned, whole, with the
// descriptors, status bytes, results and totals behind it (TxLayout),
// from where only the built frames' bytes reach buf.
int mtcp_gpu_tx_send(mtcp_gpu_ctx *ctx, const mtcp_gpu_tx_burst *burst, uint32_t n_burst,
                     const void *payload, uint64_t payload_bytes,
                     const mtcp_gpu_tx_link *links, uint32_t n_links,
                     void *buf, uint64_t buf_off, uint64_t buf_len, uint32_t off_shift,
                     uint32_t slot_bytes, uint16_t max_mss, uint32_t flags,
                     mtcp_gpu_desc *desc, uint32_t seg_cap, mtcp_gpu_tx_burst_result *res,
                     uint64_t total[2], uint8_t *status) {
    if (!ctx || !txseg_geom_ok(n_burst, n_links, buf_off, off_shift, slot_bytes, seg_cap) || !total ||
        (n_burst && (!burst || !res)) ||
        !txbuild_args_ok(ctx, seg_cap, desc, payload, payload_bytes, links, n_links, buf, buf_len, desc, off_shift,
                         flags, status))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    Stage &s = ctx->stage[0];
    const TxLayout l(n_burst, n_links, payload_bytes, buf_len, seg_cap, txseg_work(n_burst).bytes);
    int rc = stage_pinned(ctx, s, l, buf_len, 0, dl);
    if (rc != MTCP_GPU_OK) return rc;
    Call hc(s, dl, {ctx, dl});
    hc.up(l.payload(s), payload, payload_bytes, true);
    hc.up(l.burst(s), burst, l.burst.bytes);
    hc.up(l.links(s), links, l.links.bytes);
    if (hc.ok())
        hc.note(mtcp_gpu_tx_send_dev(ctx, l.burst(s), n_burst, l.payload(s), payload_bytes, l.links(s), n_links,
                                     l.image(s), buf_off, buf_len, off_shift, slot_bytes, max_mss, flags, l.seg(s),
                                     l.desc(s), seg_cap, l.res(s), l.total(s), l.status(s), l.work(s), l.work.bytes,
                                     s.stream));
    const uint8_t *image = hc.down_pinned(l.image(s), buf_len);
    rc = l.fetch(hc, s, {{desc, l.desc}, {status, l.status}, {res, l.res}, {total, l.total}});
    if (rc == MTCP_GPU_OK) copy_built(buf, image, buf_len, desc, status, seg_cap, off_shift);
    return rc;
}

// ---- pure-ACK tx segments from a walked rx batch ----------------
static_assert(sizeof(mtcp_gpu_ackgen_state) == 32 && offsetof(mtcp_gpu_ackgen_state, ip_id) == 12 &&
              offsetof(mtcp_gpu_ackgen_state, wscale_mine) == 16 && offsetof(mtcp_gpu_ackgen_state, ts_lastack_sent) == 20 &&
              offsetof(mtcp_gpu_ackgen_state, rsvd) == 24 && sizeof(mtcp_gpu_ackgen_res) == 16 &&
              offsetof(mtcp_gpu_ackgen_res, status) == 6 && offsetof(mtcp_gpu_ackgen_res, window) == 12,
              "ackgen_step.hpp reads and writes the records as dwords");
static_assert(offsetof(mtcp_gpu_rcv_place, put_len) == 12 && offsetof(mtcp_gpu_rcv_place, verdict) == 14 &&
              offsetof(mtcp_gpu_rcv_state, ts_recent) == 20 && offsetof(mtcp_gpu_rcv_state, tcp_state) == 28 &&
              offsetof(mtcp_gpu_ack_state, snd_nxt) == 0 && sizeof(mtcp_gpu_tx_seg) == 48 &&
              offsetof(mtcp_gpu_tx_seg, window) == 36 && offsetof(mtcp_gpu_tx_seg, flags) == 44,
              "ackgen_plan_kernel's loads, ackgen_record's dwords");

namespace {

bool ackgen_geom_ok(uint32_t n, uint32_t max_id, uint32_t n_links, uint64_t buf_off, uint32_t off_shift,
                    uint32_t slot_bytes, uint32_t seg_cap) {
    if (n > MTCP_GPU_GROUP_MAX_PKTS || max_id > MTCP_GPU_FLOWTAB_MAX_ID) return false;
    if (slot_bytes && slot_bytes < MTCP_GPU_ACKGEN_FRAME_LEN) return false;
    return txseg_geom_ok(0, n_links, buf_off, off_shift, slot_bytes, seg_cap);
}

bool ackgen_dev_args_ok(const mtcp_gpu_ctx *ctx, const void *d_place, uint32_t n, uint32_t max_id, const void *d_idx,
                        const void *d_seg_sid, const void *d_seg_start, const void *d_nseg, const void *d_seg_stop,
                        const void *d_ack_stop, const void *d_state, const void *d_snd, const void *d_tx,
                        uint32_t n_links, uint64_t buf_off, uint32_t off_shift, uint32_t slot_bytes,
                        const void *d_seg, const void *d_desc, uint32_t seg_cap, const void *d_ares,
                        const void *d_total, const void *d_work, uint64_t work_bytes) {
    if (!ctx || (ctx->flags & MTCP_GPU_F_COMPACT) ||
        !ackgen_geom_ok(n, max_id, n_links, buf_off, off_shift, slot_bytes, seg_cap))
        return false;
    if (!d_seg || !d_desc || !d_total ||
        (n && (!d_place || !d_idx || !d_seg_sid || !d_seg_start || !d_nseg || !d_seg_stop || !d_state || !d_snd ||
               !d_tx || !d_ares || !d_work)))
        return false;
    if (((uintptr_t)d_place & 15) || ((uintptr_t)d_idx & 3) || ((uintptr_t)d_seg_sid & 3) ||
        ((uintptr_t)d_seg_start & 3) || ((uintptr_t)d_nseg & 3) || ((uintptr_t)d_seg_stop & 3) ||
        ((uintptr_t)d_ack_stop & 3) || ((uintptr_t)d_state & 63) || ((uintptr_t)d_snd & 127) ||
        ((uintptr_t)d_tx & 31) || ((uintptr_t)d_seg & 7) || ((uintptr_t)d_desc & 7) || ((uintptr_t)d_ares & 15) ||
        ((uintptr_t)d_total & 7) || ((uintptr_t)d_work & 15))
        return false;
    return !n || work_bytes >= mg::ackgen_work(n).bytes;
}

}  // namespace

uint32_t mtcp_gpu_ackgen_lane_len(void) { return mg::kAckgenLaneMax; }

uint64_t mtcp_gpu_ackgen_work_bytes(uint32_t n, uint32_t max_id) {
    if (n > MTCP_GPU_GROUP_MAX_PKTS || max_id > MTCP_GPU_FLOWTAB_MAX_ID) return 0;
    return mg::ackgen_work(n).bytes;
}

int mtcp_gpu_ackgen_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_rcv_place *d_place, uint32_t n, uint32_t max_id,
                        const uint32_t *d_idx, const uint32_t *d_seg_sid, const uint32_t *d_seg_start,
                        const uint32_t *d_nseg, const uint32_t *d_seg_stop, const uint32_t *d_ack_stop,
                        const mtcp_gpu_rcv_state *d_state, const mtcp_gpu_ack_state *d_snd, uint32_t cur_ts,
                        mtcp_gpu_ackgen_state *d_tx, uint32_t n_links, uint64_t buf_off, uint64_t buf_len,
                        uint32_t off_shift, uint32_t slot_bytes, mtcp_gpu_tx_seg *d_seg, mtcp_gpu_desc *d_desc,
                        uint32_t seg_cap, mtcp_gpu_ackgen_res *d_ares, uint64_t *d_total, void *d_work,
                        uint64_t work_bytes, void *stream) {
    if (!ackgen_dev_args_ok(ctx, d_place, n, max_id, d_idx, d_seg_sid, d_seg_start, d_nseg, d_seg_stop, d_ack_stop,
                            d_state, d_snd, d_tx, n_links, buf_off, off_shift, slot_bytes, d_seg, d_desc, seg_cap,
                            d_ares, d_total, d_work, work_bytes))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    DeviceGuard dg(ctx->device);
    hipStream_t st = pick(ctx, stream);
    mg::AckGenParams P{};
    P.buf_off = buf_off;
    P.n = n, P.max_id = max_id, P.n_links = n_links, P.cur_ts = cur_ts, P.off_shift = off_shift;
    P.slot = mg::ackgen_slot(off_shift, slot_bytes);
    P.seg_cap = seg_cap;
    P.room = mg::ackgen_room(buf_off, buf_len, off_shift, P.slot, seg_cap);
    const mg::AckGenWork w = mg::ackgen_work(n);
    uint8_t *work = static_cast<uint8_t *>(d_work);
    mg::v4u *plan = reinterpret_cast<mg::v4u *>(work + w.plan_off);
    uint32_t *local = reinterpret_cast<uint32_t *>(work + w.local_off);
    uint32_t *part_c = reinterpret_cast<uint32_t *>(work + w.pc_off);
    uint64_t *part_b = reinterpret_cast<uint64_t *>(work + w.pb_off);
    unsigned long long *tot_b = reinterpret_cast<unsigned long long *>(work + w.tot_off);
    uint32_t *tot_c = reinterpret_cast<uint32_t *>(work + w.tot_off + 8);
    const dim3 block(mg::kBlock);
    if (n) {
        hipLaunchKernelGGL(mg::ackgen_plan_kernel<mg::kAckgenLaneMax>, dim3(w.nwg), block, 0, st, reinterpret_cast<const uint8_t *>(d_place),
                           d_idx, P, d_seg_sid, d_seg_start, d_nseg, d_seg_stop, d_ack_stop,
                           reinterpret_cast<const uint8_t *>(d_state), reinterpret_cast<const uint8_t *>(d_snd),
                           reinterpret_cast<const uint8_t *>(d_tx), plan, local, part_c, part_b);
        hipLaunchKernelGGL(mg::txseg_scan_kernel, dim3(1), block, 0, st, part_c, part_b, w.nwg, seg_cap, tot_c, tot_b);
    }
    const uint32_t lanes = std::max(seg_cap, n);
    hipLaunchKernelGGL(mg::ackgen_emit_kernel, dim3((lanes + mg::kBlock - 1) / mg::kBlock), block, 0, st, plan, local,
                       part_c, tot_c, d_nseg, w.nwg, P, d_seg_sid, reinterpret_cast<uint8_t *>(d_tx), d_seg, d_desc,
                       d_ares, d_total);
    ctx->last_kernel = "ackgen_emit_kernel";
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

int mtcp_gpu_ack_send_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_rcv_place *d_place, uint32_t n, uint32_t max_id,
                          const uint32_t *d_idx, const uint32_t *d_seg_sid, const uint32_t *d_seg_start,
                          const uint32_t *d_nseg, const uint32_t *d_seg_stop, const uint32_t *d_ack_stop,
                          const mtcp_gpu_rcv_state *d_state, const mtcp_gpu_ack_state *d_snd, uint32_t cur_ts,
                          mtcp_gpu_ackgen_state *d_tx, const mtcp_gpu_tx_link *d_links, uint32_t n_links,
                          void *d_buf, uint64_t buf_off, uint64_t buf_len, uint32_t off_shift,
                          uint32_t slot_bytes, uint32_t flags, mtcp_gpu_tx_seg *d_seg, mtcp_gpu_desc *d_desc,
                          uint32_t seg_cap, mtcp_gpu_ackgen_res *d_ares, uint64_t *d_total, uint8_t *d_status,
                          void *d_work, uint64_t work_bytes, void *stream) {
    // both calls' checks before either launches; the builder's payload is the
    // workspace pointer with no bytes (never dereferenced for payload_len == 0)
    if (!ackgen_dev_args_ok(ctx, d_place, n, max_id, d_idx, d_seg_sid, d_seg_start, d_nseg, d_seg_stop, d_ack_stop,
                            d_state, d_snd, d_tx, n_links, buf_off, off_shift, slot_bytes, d_seg, d_desc, seg_cap,
                            d_ares, d_total, d_work, work_bytes) ||
        !txbuild_args_ok(ctx, seg_cap, d_seg, d_work, 0, d_links, n_links, d_buf, buf_len, d_desc, off_shift, flags,
                         d_status) ||
        ((uintptr_t)d_links & 3))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    const int rc = mtcp_gpu_ackgen_dev(ctx, d_place, n, max_id, d_idx, d_seg_sid, d_seg_start, d_nseg, d_seg_stop,
                                       d_ack_stop, d_state, d_snd, cur_ts, d_tx, n_links, buf_off, buf_len, off_shift,
                                       slot_bytes, d_seg, d_desc, seg_cap, d_ares, d_total, d_work, work_bytes,
                                       stream);
    if (rc != MTCP_GPU_OK) return rc;
    return mtcp_gpu_tx_build_dev(ctx, d_seg, seg_cap, d_work, 0, d_links, n_links, d_buf, buf_len, d_desc, off_shift,
                                 0, flags, d_status, stream);
}

int mtcp_gpu_ackgen(mtcp_gpu_ctx *ctx, const mtcp_gpu_rcv_place *place, uint32_t n, uint32_t max_id,
                    const uint32_t *idx, const uint32_t *seg_sid, const uint32_t *seg_start, const uint32_t *nseg,
                    const uint32_t *seg_stop, const uint32_t *ack_stop, const mtcp_gpu_rcv_state *state,
                    const mtcp_gpu_ack_state *snd, uint32_t cur_ts, mtcp_gpu_ackgen_state *tx, uint32_t n_links,
                    uint64_t buf_off, uint64_t buf_len, uint32_t off_shift, uint32_t slot_bytes,
                    mtcp_gpu_tx_seg *seg, mtcp_gpu_desc *desc, uint32_t seg_cap, mtcp_gpu_ackgen_res *ares,
                    uint64_t total[2]) {
    if (!ctx || (ctx->flags & MTCP_GPU_F_COMPACT) ||
        !ackgen_geom_ok(n, max_id, n_links, buf_off, off_shift, slot_bytes, seg_cap) || !seg || !desc || !total ||
        (n && (!place || !idx || !seg_sid || !seg_start || !nseg || !seg_stop || !state || !snd || !tx || !ares)))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    const uint32_t m = n ? std::min(nseg[0], n) : 0u;
    const AckgenLayout l(false, n, max_id, m, ack_stop != nullptr, seg_cap, mg::ackgen_work(n).bytes);
    Stage &s = ctx->stage[0];
    int rc = stage_pinned(ctx, s, l, 0, 0, dl);
    if (rc != MTCP_GPU_OK) return rc;
    Call hc(s, dl, {ctx, dl});
    if (n) {
        hc.up(l.in_rec(s), place, l.in_rec.bytes);
        l.g.up(hc, s, idx, seg_sid, seg_start, &m, seg_stop, ack_stop);
        hc.up(l.snd(s), snd, l.snd.bytes);
        hc.up(l.state(s), state, l.state.bytes);
        hc.up(l.tx(s), tx, l.tx.bytes);
    }
    if (hc.ok())
        hc.note(mtcp_gpu_ackgen_dev(ctx, l.in_rec(s), n, max_id, l.g.idx(s), l.g.seg_sid(s), l.g.seg_start(s),
                                    l.g.nseg(s), l.g.seg_stop(s), ack_stop ? l.g.ack_stop(s) : nullptr, l.state(s),
                                    l.snd(s), cur_ts, l.tx(s), n_links, buf_off, buf_len, off_shift, slot_bytes,
                                    l.seg(s), l.desc(s), seg_cap, l.res(s), l.total(s), l.work(s), l.work.bytes,
                                    s.stream));
    return l.fetch(hc, s, {{tx, l.tx}, {seg, l.seg}, {desc, l.desc},
                           {ares, l.res, (uint64_t)m * sizeof(mtcp_gpu_ackgen_res)}, {total, l.total}});
}

// ---- data tx segments from a walked rx batch ---------------------
static_assert(sizeof(mtcp_gpu_datagen_state) == 16 && offsetof(mtcp_gpu_datagen_state, sb_base_seq) == 8 &&
              offsetof(mtcp_gpu_datagen_state, on_send_list) == 12 && offsetof(mtcp_gpu_datagen_state, rsvd) == 14 &&
              sizeof(mtcp_gpu_datagen_res) == 16 && offsetof(mtcp_gpu_datagen_res, status) == 12 &&
              offsetof(mtcp_gpu_datagen_res, flags) == 14,
              "datagen_step.hpp reads and writes the records as dwords");
static_assert(offsetof(mtcp_gpu_ack_rec, flags) == 12 && offsetof(mtcp_gpu_ack_state, peer_wnd) == 12 &&
              offsetof(mtcp_gpu_ack_state, cwnd) == 28 && offsetof(mtcp_gpu_ack_state, rto) == 36 &&
              offsetof(mtcp_gpu_ack_state, ts_rto) == 40 && offsetof(mtcp_gpu_ack_state, sb_head_seq) == 64 &&
              offsetof(mtcp_gpu_ack_state, mss) == 76 && offsetof(mtcp_gpu_ack_state, tcp_state) == 80 &&
              offsetof(mtcp_gpu_ack_state, on_rto) == 85 && offsetof(mtcp_gpu_ack_state, user) == 88 &&
              offsetof(mtcp_gpu_tx_burst, len) == 36 && offsetof(mtcp_gpu_tx_burst, tcp_window) == 52 &&
              offsetof(mtcp_gpu_tx_burst, mss) == 56,
              "datagen_burst_kernel's loads, datagen_burst's dwords, datagen_commit_kernel's stores");

namespace {

bool datagen_geom_ok(uint32_t n, uint32_t max_id, uint32_t n_links, uint64_t buf_off, uint32_t off_shift,
                     uint32_t slot_bytes, uint32_t seg_cap) {
    if (n > MTCP_GPU_GROUP_MAX_PKTS || n > MTCP_GPU_TXSEG_MAX_BURSTS || max_id > MTCP_GPU_FLOWTAB_MAX_ID) return false;
    if (slot_bytes && slot_bytes < 67) return false;
    return txseg_geom_ok(n, n_links, buf_off, off_shift, slot_bytes, seg_cap);
}

uint64_t datagen_work_total(uint32_t n) { return mg::datagen_work(n).f8_off + txseg_work(n).bytes; }

bool datagen_dev_args_ok(const mtcp_gpu_ctx *ctx, const void *d_ack, const void *d_ack_stop, uint32_t n,
                         uint32_t max_id, const void *d_idx, const void *d_seg_sid, const void *d_seg_start,
                         const void *d_nseg, const void *d_seg_stop, const void *d_state, const void *d_snd,
                         const void *d_tx, const void *d_dtx, uint32_t n_links, uint64_t buf_off, uint32_t off_shift,
                         uint32_t slot_bytes, const void *d_seg, const void *d_desc, uint32_t seg_cap,
                         const void *d_dres, const void *d_total, const void *d_work, uint64_t work_bytes) {
    if (!ctx || (ctx->flags & MTCP_GPU_F_COMPACT) ||
        !datagen_geom_ok(n, max_id, n_links, buf_off, off_shift, slot_bytes, seg_cap))
        return false;
    if (!d_seg || !d_desc || !d_total || !d_work || (!d_ack != !d_ack_stop) ||
        (n && (!d_idx || !d_seg_sid || !d_seg_start || !d_nseg || !d_seg_stop || !d_state || !d_snd || !d_tx ||
               !d_dtx || !d_dres)))
        return false;
    if (((uintptr_t)d_ack & 15) || ((uintptr_t)d_ack_stop & 3) || ((uintptr_t)d_idx & 3) ||
        ((uintptr_t)d_seg_sid & 3) || ((uintptr_t)d_seg_start & 3) || ((uintptr_t)d_nseg & 3) ||
        ((uintptr_t)d_seg_stop & 3) || ((uintptr_t)d_state & 63) || ((uintptr_t)d_snd & 127) ||
        ((uintptr_t)d_tx & 31) || ((uintptr_t)d_dtx & 15) || ((uintptr_t)d_seg & 7) || ((uintptr_t)d_desc & 7) ||
        ((uintptr_t)d_dres & 15) || ((uintptr_t)d_total & 7) || ((uintptr_t)d_work & 15))
        return false;
    return work_bytes >= datagen_work_total(n);
}

}  // namespace

uint32_t mtcp_gpu_datagen_lane_len(void) { return mg::kDatagenLaneMax; }

uint64_t mtcp_gpu_datagen_work_bytes(uint32_t n, uint32_t max_id) {
    if (n > MTCP_GPU_GROUP_MAX_PKTS || n > MTCP_GPU_TXSEG_MAX_BURSTS || max_id > MTCP_GPU_FLOWTAB_MAX_ID) return 0;
    return datagen_work_total(n);
}

int mtcp_gpu_datagen_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_ack_rec *d_ack, const uint32_t *d_ack_stop, uint32_t n,
                         uint32_t max_id, const uint32_t *d_idx, const uint32_t *d_seg_sid,
                         const uint32_t *d_seg_start, const uint32_t *d_nseg, const uint32_t *d_seg_stop,
                         const mtcp_gpu_rcv_state *d_state, mtcp_gpu_ack_state *d_snd, mtcp_gpu_ackgen_state *d_tx,
                         mtcp_gpu_datagen_state *d_dtx, uint32_t cur_ts, uint64_t payload_bytes, uint32_t n_links,
                         uint64_t buf_off, uint64_t buf_len, uint32_t off_shift, uint32_t slot_bytes,
                         uint16_t max_mss, mtcp_gpu_tx_seg *d_seg, mtcp_gpu_desc *d_desc, uint32_t seg_cap,
                         mtcp_gpu_datagen_res *d_dres, uint64_t *d_total, void *d_work, uint64_t work_bytes,
                         void *stream) {
    if (!datagen_dev_args_ok(ctx, d_ack, d_ack_stop, n, max_id, d_idx, d_seg_sid, d_seg_start, d_nseg, d_seg_stop,
                             d_state, d_snd, d_tx, d_dtx, n_links, buf_off, off_shift, slot_bytes, d_seg, d_desc,
                             seg_cap, d_dres, d_total, d_work, work_bytes))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    DeviceGuard dg(ctx->device);
    hipStream_t st = pick(ctx, stream);
    const mg::DataGenWork w = mg::datagen_work(n);
    uint8_t *work = static_cast<uint8_t *>(d_work);
    mtcp_gpu_tx_burst *burst = reinterpret_cast<mtcp_gpu_tx_burst *>(work + w.burst_off);
    mtcp_gpu_tx_burst_result *f8res = reinterpret_cast<mtcp_gpu_tx_burst_result *>(work + w.res_off);
    uint32_t *park = reinterpret_cast<uint32_t *>(work + w.park_off);
    const mg::DataGenParams P{n, max_id, n_links, cur_ts};
    const dim3 block(mg::kBlock), grid((n + mg::kBlock - 1) / mg::kBlock);
    if (n) {
        hipLaunchKernelGGL(mg::datagen_burst_kernel<mg::kDatagenLaneMax>, grid, block, 0, st,
                           reinterpret_cast<const uint8_t *>(d_ack), d_idx, P, d_seg_sid, d_seg_start, d_nseg,
                           d_seg_stop, d_ack_stop, reinterpret_cast<const uint8_t *>(d_state),
                           reinterpret_cast<const uint8_t *>(d_snd), reinterpret_cast<const uint8_t *>(d_tx),
                           reinterpret_cast<const uint8_t *>(d_dtx), reinterpret_cast<uint8_t *>(burst), park);
        if (!HIP_OK(hipGetLastError())) return MTCP_GPU_EIO;
    }
    const int rc = mtcp_gpu_tx_segment_dev(ctx, burst, n, payload_bytes, n_links, buf_off, buf_len, off_shift,
                                           slot_bytes, max_mss, d_seg, d_desc, seg_cap, f8res, d_total,
                                           work + w.f8_off, work_bytes - w.f8_off, st);
    if (rc != MTCP_GPU_OK || !n) return rc;
    hipLaunchKernelGGL(mg::datagen_commit_kernel, grid, block, 0, st, park, reinterpret_cast<const uint8_t *>(f8res), P,
                       d_seg_sid, d_nseg, reinterpret_cast<uint8_t *>(d_snd), reinterpret_cast<uint8_t *>(d_tx),
                       reinterpret_cast<uint8_t *>(d_dtx), d_dres);
    ctx->last_kernel = "datagen_commit_kernel";
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

int mtcp_gpu_data_send_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_ack_rec *d_ack, const uint32_t *d_ack_stop, uint32_t n,
                           uint32_t max_id, const uint32_t *d_idx, const uint32_t *d_seg_sid,
                           const uint32_t *d_seg_start, const uint32_t *d_nseg, const uint32_t *d_seg_stop,
                           const mtcp_gpu_rcv_state *d_state, mtcp_gpu_ack_state *d_snd, mtcp_gpu_ackgen_state *d_tx,
                           mtcp_gpu_datagen_state *d_dtx, uint32_t cur_ts, const void *d_payload,
                           uint64_t payload_bytes, const mtcp_gpu_tx_link *d_links, uint32_t n_links, void *d_buf,
                           uint64_t buf_off, uint64_t buf_len, uint32_t off_shift, uint32_t slot_bytes,
                           uint16_t max_mss, uint32_t flags, mtcp_gpu_tx_seg *d_seg, mtcp_gpu_desc *d_desc,
                           uint32_t seg_cap, mtcp_gpu_datagen_res *d_dres, uint64_t *d_total, uint8_t *d_status,
                           void *d_work, uint64_t work_bytes, void *stream) {
    // both calls' checks before either launches
    if (!datagen_dev_args_ok(ctx, d_ack, d_ack_stop, n, max_id, d_idx, d_seg_sid, d_seg_start, d_nseg, d_seg_stop,
                             d_state, d_snd, d_tx, d_dtx, n_links, buf_off, off_shift, slot_bytes, d_seg, d_desc,
                             seg_cap, d_dres, d_total, d_work, work_bytes) ||
        !txbuild_args_ok(ctx, seg_cap, d_seg, d_payload, payload_bytes, d_links, n_links, d_buf, buf_len, d_desc,
                         off_shift, flags, d_status) ||
        ((uintptr_t)d_links & 3))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    const int rc = mtcp_gpu_datagen_dev(ctx, d_ack, d_ack_stop, n, max_id, d_idx, d_seg_sid, d_seg_start, d_nseg,
                                        d_seg_stop, d_state, d_snd, d_tx, d_dtx, cur_ts, payload_bytes, n_links,
                                        buf_off, buf_len, off_shift, slot_bytes, max_mss, d_seg, d_desc, seg_cap,
                                        d_dres, d_total, d_work, work_bytes, stream);
    if (rc != MTCP_GPU_OK) return rc;
    return mtcp_gpu_tx_build_dev(ctx, d_seg, seg_cap, d_payload, payload_bytes, d_links, n_links, d_buf, buf_len,
                                 d_desc, off_shift, max_mss, flags, d_status, stream);
}

int mtcp_gpu_datagen(mtcp_gpu_ctx *ctx, const mtcp_gpu_ack_rec *ack, const uint32_t *ack_stop, uint32_t n,
                     uint32_t max_id, const uint32_t *idx, const uint32_t *seg_sid, const uint32_t *seg_start,
                     const uint32_t *nseg, const uint32_t *seg_stop, const mtcp_gpu_rcv_state *state,
                     mtcp_gpu_ack_state *snd, mtcp_gpu_ackgen_state *tx, mtcp_gpu_datagen_state *dtx, uint32_t cur_ts,
                     uint64_t payload_bytes, uint32_t n_links, uint64_t buf_off, uint64_t buf_len,
                     uint32_t off_shift, uint32_t slot_bytes, uint16_t max_mss, mtcp_gpu_tx_seg *seg,
                     mtcp_gpu_desc *desc, uint32_t seg_cap, mtcp_gpu_datagen_res *dres, uint64_t total[2]) {
    if (!ctx || (ctx->flags & MTCP_GPU_F_COMPACT) ||
        !datagen_geom_ok(n, max_id, n_links, buf_off, off_shift, slot_bytes, seg_cap) || !seg || !desc || !total ||
        (!ack != !ack_stop) ||
        (n && (!idx || !seg_sid || !seg_start || !nseg || !seg_stop || !state || !snd || !tx || !dtx || !dres)))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    const uint32_t m = n ? std::min(nseg[0], n) : 0u;
    const DatagenLayout l(true, n, max_id, m, ack != nullptr, seg_cap, datagen_work_total(n));
    Stage &s = ctx->stage[0];
    int rc = stage_pinned(ctx, s, l, 0, 0, dl);
    if (rc != MTCP_GPU_OK) return rc;
    Call hc(s, dl, {ctx, dl});
    if (n) {
        if (ack) hc.up(l.in_rec(s), ack, l.in_rec.bytes);
        l.g.up(hc, s, idx, seg_sid, seg_start, &m, seg_stop, ack_stop);
        hc.up(l.state(s), state, l.state.bytes);
        hc.up(l.snd(s), snd, l.snd.bytes);
        hc.up(l.tx(s), tx, l.tx.bytes);
        hc.up(l.dtx(s), dtx, l.dtx.bytes);
    }
    if (hc.ok())
        hc.note(mtcp_gpu_datagen_dev(ctx, ack ? l.in_rec(s) : nullptr, ack_stop ? l.g.ack_stop(s) : nullptr, n, max_id,
                                     l.g.idx(s), l.g.seg_sid(s), l.g.seg_start(s), l.g.nseg(s), l.g.seg_stop(s),
                                     l.state(s), l.snd(s), l.tx(s), l.dtx(s), cur_ts, payload_bytes, n_links, buf_off,
                                     buf_len, off_shift, slot_bytes, max_mss, l.seg(s), l.desc(s), seg_cap, l.res(s),
                                     l.total(s), l.work(s), l.work.bytes, s.stream));
    return l.fetch(hc, s, {{snd, l.snd}, {tx, l.tx}, {dtx, l.dtx}, {seg, l.seg}, {desc, l.desc},
                           {dres, l.res, (uint64_t)m * sizeof(mtcp_gpu_datagen_res)}, {total, l.total}});
}

// ---- the retransmission-timeout sweep over device send states ----
static_assert(sizeof(mtcp_gpu_rto_rec) == 16 && offsetof(mtcp_gpu_rto_rec, rto) == 4 &&
              offsetof(mtcp_gpu_rto_rec, nrtx) == 8 && offsetof(mtcp_gpu_rto_rec, verdict) == 9 &&
              offsetof(mtcp_gpu_rto_rec, flags) == 10 && offsetof(mtcp_gpu_rto_rec, rsvd1) == 12,
              "rto_step.hpp writes the record as dwords");
static_assert(offsetof(mtcp_gpu_ack_state, snd_una) == 4 && offsetof(mtcp_gpu_ack_state, ssthresh) == 32 &&
              offsetof(mtcp_gpu_ack_state, srtt) == 44 && offsetof(mtcp_gpu_ack_state, rttvar) == 56 &&
              offsetof(mtcp_gpu_ack_state, sb_len) == 68 && offsetof(mtcp_gpu_ack_state, nrtx) == 84 &&
              offsetof(mtcp_gpu_ack_state, has_sndbuf) == 86,
              "rto_lane_due's and rto_handle's loads and stores");

namespace {

bool rto_geom_ok(uint32_t max_id, uint32_t cap) {
    return cap != 0 && cap <= MTCP_GPU_TXSEG_MAX_BURSTS && max_id <= MTCP_GPU_FLOWTAB_MAX_ID;
}

bool rto_dev_args_ok(const mtcp_gpu_ctx *ctx, uint32_t max_id, const void *d_snd, const void *d_dtx, uint32_t cap,
                     const void *d_rto, const void *d_seg_sid, const void *d_seg_start, const void *d_seg_stop,
                     const void *d_nseg, const void *d_total, const void *d_work, uint64_t work_bytes) {
    if (!ctx || !rto_geom_ok(max_id, cap)) return false;
    if (!d_snd || !d_dtx || !d_rto || !d_seg_sid || !d_seg_start || !d_seg_stop || !d_nseg || !d_total || !d_work)
        return false;
    if (((uintptr_t)d_snd & 127) || ((uintptr_t)d_dtx & 15) || ((uintptr_t)d_rto & 15) ||
        ((uintptr_t)d_seg_sid & 3) || ((uintptr_t)d_seg_start & 3) || ((uintptr_t)d_seg_stop & 3) ||
        ((uintptr_t)d_nseg & 3) || ((uintptr_t)d_total & 7) || ((uintptr_t)d_work & 15))
        return false;
    return work_bytes >= mg::rto_sweep_work(max_id).bytes;
}

}  // namespace

uint32_t mtcp_gpu_rto_sweep_tile(void) { return mg::kRtoTile; }

uint64_t mtcp_gpu_rto_sweep_work_bytes(uint32_t max_id, uint32_t cap) {
    if (!rto_geom_ok(max_id, cap)) return 0;
    return mg::rto_sweep_work(max_id).bytes;
}

int mtcp_gpu_rto_sweep_dev(mtcp_gpu_ctx *ctx, uint32_t max_id, mtcp_gpu_ack_state *d_snd,
                           mtcp_gpu_datagen_state *d_dtx, uint32_t cur_ts, uint32_t cap, mtcp_gpu_rto_rec *d_rto,
                           uint32_t *d_seg_sid, uint32_t *d_seg_start, uint32_t *d_seg_stop, uint32_t *d_nseg,
                           uint64_t *d_total, void *d_work, uint64_t work_bytes, void *stream) {
    if (!rto_dev_args_ok(ctx, max_id, d_snd, d_dtx, cap, d_rto, d_seg_sid, d_seg_start, d_seg_stop, d_nseg, d_total,
                         d_work, work_bytes))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    DeviceGuard dg(ctx->device);
    hipStream_t st = pick(ctx, stream);
    const mg::RtoSweepWork w = mg::rto_sweep_work(max_id);
    const mg::RtoSweepParams P{max_id, cap, cur_ts};
    uint8_t *snd = reinterpret_cast<uint8_t *>(d_snd), *dtx = reinterpret_cast<uint8_t *>(d_dtx);
    const dim3 block(mg::kBlock);
    if (w.ntiles == 1 && cap <= mg::kRtoTile) {
        hipLaunchKernelGGL(mg::rto_one_kernel, dim3(1), block, 0, st, P, snd, dtx, d_rto, d_seg_sid,
                           d_seg_start, d_seg_stop, d_nseg, d_total);
        ctx->last_kernel = "rto_one_kernel";
        return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
    }
    uint8_t *work = static_cast<uint8_t *>(d_work);
    uint64_t *ballots = reinterpret_cast<uint64_t *>(work + w.ballot_off);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(work + w.cnt_off);
    uint32_t *tot = reinterpret_cast<uint32_t *>(work + w.tot_off);
    hipLaunchKernelGGL(mg::rto_count_kernel, dim3(w.ntiles), block, 0, st, snd, P, ballots, cnt);
    hipLaunchKernelGGL(mg::steer_scan_kernel, dim3(1), block, 0, st, cnt, w.nwaves, tot);
    hipLaunchKernelGGL(mg::rto_emit_kernel, dim3(w.ntiles), block, 0, st, ballots, cnt, tot, P, snd, dtx, d_rto,
                       d_seg_sid, d_seg_start, d_seg_stop, d_nseg, d_total);
    ctx->last_kernel = "rto_emit_kernel";
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

int mtcp_gpu_rto_send_dev(mtcp_gpu_ctx *ctx, uint32_t max_id, mtcp_gpu_ack_state *d_snd,
                          mtcp_gpu_datagen_state *d_dtx, uint32_t cur_ts, uint32_t cap, mtcp_gpu_rto_rec *d_rto,
                          uint32_t *d_seg_sid, uint32_t *d_seg_start, uint32_t *d_seg_stop, uint32_t *d_nseg,
                          uint64_t *d_total, void *d_rwork, uint64_t rwork_bytes, const uint32_t *d_idx,
                          const mtcp_gpu_rcv_state *d_state, mtcp_gpu_ackgen_state *d_tx, const void *d_payload,
                          uint64_t payload_bytes, const mtcp_gpu_tx_link *d_links, uint32_t n_links, void *d_buf,
                          uint64_t buf_off, uint64_t buf_len, uint32_t off_shift, uint32_t slot_bytes,
                          uint16_t max_mss, uint32_t flags, mtcp_gpu_tx_seg *d_seg, mtcp_gpu_desc *d_desc,
                          uint32_t seg_cap, mtcp_gpu_datagen_res *d_dres, uint64_t *d_dtotal, uint8_t *d_status,
                          void *d_work, uint64_t work_bytes, void *stream) {
    // both calls' checks before either launches
    if (!rto_dev_args_ok(ctx, max_id, d_snd, d_dtx, cap, d_rto, d_seg_sid, d_seg_start, d_seg_stop, d_nseg, d_total,
                         d_rwork, rwork_bytes) ||
        !datagen_dev_args_ok(ctx, nullptr, nullptr, cap, max_id, d_idx, d_seg_sid, d_seg_start, d_nseg, d_seg_stop,
                             d_state, d_snd, d_tx, d_dtx, n_links, buf_off, off_shift, slot_bytes, d_seg, d_desc,
                             seg_cap, d_dres, d_dtotal, d_work, work_bytes) ||
        !txbuild_args_ok(ctx, seg_cap, d_seg, d_payload, payload_bytes, d_links, n_links, d_buf, buf_len, d_desc,
                         off_shift, flags, d_status) ||
        ((uintptr_t)d_links & 3))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    const int rc = mtcp_gpu_rto_sweep_dev(ctx, max_id, d_snd, d_dtx, cur_ts, cap, d_rto, d_seg_sid, d_seg_start,
                                          d_seg_stop, d_nseg, d_total, d_rwork, rwork_bytes, stream);
    if (rc != MTCP_GPU_OK) return rc;
    return mtcp_gpu_data_send_dev(ctx, nullptr, nullptr, cap, max_id, d_idx, d_seg_sid, d_seg_start, d_nseg,
                                  d_seg_stop, d_state, d_snd, d_tx, d_dtx, cur_ts, d_payload, payload_bytes, d_links,
                                  n_links, d_buf, buf_off, buf_len, off_shift, slot_bytes, max_mss, flags, d_seg,
                                  d_desc, seg_cap, d_dres, d_dtotal, d_status, d_work, work_bytes, stream);
}

int mtcp_gpu_rto_sweep(mtcp_gpu_ctx *ctx, uint32_t max_id, mtcp_gpu_ack_state *snd, mtcp_gpu_datagen_state *dtx,
                       uint32_t cur_ts, uint32_t cap, mtcp_gpu_rto_rec *rto, uint32_t *seg_sid, uint32_t *seg_start,
                       uint32_t *seg_stop, uint32_t *nseg, uint64_t total[2]) {
    if (!ctx || !rto_geom_ok(max_id, cap) || !snd || !dtx || !rto || !seg_sid || !seg_start || !seg_stop || !nseg ||
        !total)
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    const RtoLayout l(max_id, cap, mg::rto_sweep_work(max_id).bytes);
    Stage &s = ctx->stage[0];
    int rc = stage_pinned(ctx, s, l, 0, 0, dl);
    if (rc != MTCP_GPU_OK) return rc;
    Call hc(s, dl, {ctx, dl});
    hc.up(l.snd(s), snd, l.snd.bytes);
    hc.up(l.dtx(s), dtx, l.dtx.bytes);
    if (hc.ok())
        hc.note(mtcp_gpu_rto_sweep_dev(ctx, max_id, l.snd(s), l.dtx(s), cur_ts, cap, l.rto(s), l.seg_sid(s),
                                       l.seg_start(s), l.seg_stop(s), l.nseg(s), l.total(s), l.work(s), l.work.bytes,
                                       s.stream));
    const uint8_t *h = hc.down_pinned(s.d_buf + l.back_off, l.back_bytes());
    if ((rc = hc.finish()) != MTCP_GPU_OK) return rc;
    l.copy_out(h, {{nseg, l.nseg}});
    const uint32_t handled = std::min(nseg[0], cap);
    l.copy_out(h, {{snd, l.snd}, {dtx, l.dtx}, {rto, l.rto, (uint64_t)handled * sizeof(mtcp_gpu_rto_rec)},
                   {seg_sid, l.seg_sid, (uint64_t)handled * sizeof(uint32_t)}, {seg_start, l.seg_start},
                   {seg_stop, l.seg_stop}, {total, l.total}});
    return MTCP_GPU_OK;
}

// ---- the batched application read out of device receive buffers ----
static_assert(sizeof(mtcp_gpu_rcvread_req) == 32 && offsetof(mtcp_gpu_rcvread_req, len) == 4 &&
              offsetof(mtcp_gpu_rcvread_req, dst_off) == 8 && offsetof(mtcp_gpu_rcvread_req, flags) == 16 &&
              offsetof(mtcp_gpu_rcvread_req, rsvd) == 20,
              "rcvread_step.hpp reads the request as dwords");
static_assert(sizeof(mtcp_gpu_rcvread_res) == 16 && offsetof(mtcp_gpu_rcvread_res, copylen) == 4 &&
              offsetof(mtcp_gpu_rcvread_res, rcv_wnd) == 8 && offsetof(mtcp_gpu_rcvread_res, verdict) == 12 &&
              offsetof(mtcp_gpu_rcvread_res, flags) == 13 && offsetof(mtcp_gpu_rcvread_res, rsvd) == 14,
              "rcvread_step.hpp writes the record as dwords");
static_assert(offsetof(mtcp_gpu_rcv_state, rcv_wnd) == 4 && offsetof(mtcp_gpu_rcv_state, head_seq) == 8 &&
              offsetof(mtcp_gpu_rcv_state, merged_len) == 12 && offsetof(mtcp_gpu_rcv_state, size) == 16 &&
              offsetof(mtcp_gpu_rcv_state, tcp_state) == 28 && offsetof(mtcp_gpu_rcv_state, nfrag) == 30 &&
              offsetof(mtcp_gpu_rcv_state, frag) == 32 && offsetof(mtcp_gpu_rcv_buf, size) == 8 &&
              offsetof(mtcp_gpu_rcv_buf, head_offset) == 12 && offsetof(mtcp_gpu_rcv_buf, last_len) == 20 &&
              sizeof(mtcp_gpu_ackgen_state) == 32 && offsetof(mtcp_gpu_ackgen_state, need_wnd_adv) == 19 &&
              sizeof(mtcp_gpu_ack_state) == 128 && offsetof(mtcp_gpu_ack_state, eff_mss) == 78,
              "read_step's dwords and rcvread_plan_kernel's loads and stores");

namespace {

bool rcvread_geom_ok(uint32_t n, uint32_t max_id) {
    return n <= MTCP_GPU_GROUP_MAX_PKTS && max_id <= MTCP_GPU_FLOWTAB_MAX_ID;
}

// what both forms ask of the device-resident arguments
bool rcvread_mirrors_ok(const mtcp_gpu_ctx *ctx, uint32_t n, uint32_t max_id, const void *d_state, const void *d_rbuf,
                        const void *d_tx, const void *d_snd, const void *d_arena, uint64_t arena_bytes) {
    if (!ctx || !rcvread_geom_ok(n, max_id) || (n && (!d_state || !d_rbuf || !d_arena)) || !d_tx != !d_snd) return false;
    return !(((uintptr_t)d_state & 63) || ((uintptr_t)d_snd & 127) || ((uintptr_t)d_rbuf & 31) ||
             ((uintptr_t)d_tx & 31) || ((uintptr_t)d_arena & 15) || (arena_bytes & 15));
}

// The five launches; d_pack: the synchronous form's gather offsets, or nullptr.
int rcvread_launch(mtcp_gpu_ctx *ctx, const mtcp_gpu_rcvread_req *d_req, uint32_t n, uint32_t max_id,
                   mtcp_gpu_rcv_state *d_state, mtcp_gpu_rcv_buf *d_rbuf, mtcp_gpu_ackgen_state *d_tx,
                   const mtcp_gpu_ack_state *d_snd, const void *d_arena, uint64_t arena_bytes, void *d_dst,
                   uint64_t dst_bytes, uint64_t store_bytes, const uint64_t *d_pack, mtcp_gpu_rcvread_res *d_rres,
                   uint64_t *d_total, void *d_work, hipStream_t st) {
    const mg::ReadWork w = mg::read_work(n, max_id);
    const mg::ReadParams P{n, max_id, arena_bytes, dst_bytes};
    uint8_t *work = static_cast<uint8_t *>(d_work);
    uint32_t *claim = reinterpret_cast<uint32_t *>(work + w.claim_off);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(work + w.cnt_off);
    uint32_t *part = reinterpret_cast<uint32_t *>(work + w.part_off);
    uint32_t *tot = reinterpret_cast<uint32_t *>(work + w.tot_off);
    uint4 *plan = reinterpret_cast<uint4 *>(work + w.plan_off);
    const uint4 *req = reinterpret_cast<const uint4 *>(d_req);
    const dim3 block(mg::kBlock), grid(w.nwg);
    hipLaunchKernelGGL(mg::rcvread_clear_kernel, grid, block, 0, st, req, P, claim, d_total);
    hipLaunchKernelGGL(mg::rcvread_claim_kernel, grid, block, 0, st, req, P, claim);
    hipLaunchKernelGGL(mg::rcvread_plan_kernel, grid, block, 0, st, req, P, claim, reinterpret_cast<uint4 *>(d_state),
                       reinterpret_cast<uint32_t *>(d_rbuf), reinterpret_cast<uint8_t *>(d_tx),
                       reinterpret_cast<const uint8_t *>(d_snd), d_pack, reinterpret_cast<uint4 *>(d_rres), d_total,
                       cnt, part, plan);
    hipLaunchKernelGGL(mg::steer_scan_kernel, dim3(1), block, 0, st, part, w.nwg, tot);
    // a wave per unit up to eight workgroups a CU; the grid walks what is beyond with its stride.  The units of
    // disjoint ranges: one per request for a ragged end, and the bytes that can be stored
    const uint64_t units = (uint64_t)n + std::min(store_bytes, arena_bytes) / mg::kReadUnit;
    const uint64_t wgs = (units + mg::kWavesPerBlock - 1) / mg::kWavesPerBlock;
    const uint32_t cgrid = (uint32_t)std::min<uint64_t>(wgs, (uint64_t)ctx->num_cu * 8);
    hipLaunchKernelGGL(mg::rcvread_copy_kernel, dim3(cgrid), block, 0, st, cnt, part, tot, w.nwg, plan,
                       (uint64_t)(uintptr_t)d_arena, (uint64_t)(uintptr_t)d_dst);
    ctx->last_kernel = "rcvread_copy_kernel";
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

}  // namespace

uint32_t mtcp_gpu_rcvread_tile(void) { return mg::kReadUnit; }

uint64_t mtcp_gpu_rcvread_work_bytes(uint32_t n, uint32_t max_id) {
    if (!rcvread_geom_ok(n, max_id)) return 0;
    return mg::read_work(n, max_id).bytes;
}

int mtcp_gpu_rcvread_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_rcvread_req *d_req, uint32_t n, uint32_t max_id,
                         mtcp_gpu_rcv_state *d_state, mtcp_gpu_rcv_buf *d_rbuf, mtcp_gpu_ackgen_state *d_tx,
                         const mtcp_gpu_ack_state *d_snd, const void *d_arena, uint64_t arena_bytes, void *d_dst,
                         uint64_t dst_bytes, mtcp_gpu_rcvread_res *d_rres, uint64_t *d_total, void *d_work,
                         uint64_t work_bytes, void *stream) {
    if (!rcvread_mirrors_ok(ctx, n, max_id, d_state, d_rbuf, d_tx, d_snd, d_arena, arena_bytes) ||
        (n && (!d_req || !d_dst || !d_rres || !d_total || !d_work)) || ((uintptr_t)d_req & 15) ||
        ((uintptr_t)d_dst & 15) || ((uintptr_t)d_rres & 15) || ((uintptr_t)d_total & 7) || ((uintptr_t)d_work & 15) ||
        (n && work_bytes < mg::read_work(n, max_id).bytes))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    return rcvread_launch(ctx, d_req, n, max_id, d_state, d_rbuf, d_tx, d_snd, d_arena, arena_bytes, d_dst, dst_bytes,
                          dst_bytes, nullptr, d_rres, d_total, d_work, pick(ctx, stream));
}

int mtcp_gpu_rcvread(mtcp_gpu_ctx *ctx, const mtcp_gpu_rcvread_req *req, uint32_t n, uint32_t max_id,
                     mtcp_gpu_rcv_state *d_state, mtcp_gpu_rcv_buf *d_rbuf, mtcp_gpu_ackgen_state *d_tx,
                     const mtcp_gpu_ack_state *d_snd, const void *d_arena, uint64_t arena_bytes, void *dst,
                     uint64_t dst_bytes, mtcp_gpu_rcvread_res *rres, uint64_t total[2]) {
    if (!rcvread_mirrors_ok(ctx, n, max_id, d_state, d_rbuf, d_tx, d_snd, d_arena, arena_bytes) ||
        (n && (!req || !dst || !rres || !total)))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    // the gather: request i's bytes at pack[i] of the stage, len bytes each, 16 B aligned.  The bound is tested
    // before the table is allocated, and no exception leaves a C entry point
    uint64_t gather = 0;
    for (uint32_t i = 0; i < n; ++i)
        if ((gather += pad16(req[i].len)) > MTCP_GPU_RCVREAD_HOST_MAX_BYTES) return MTCP_GPU_EINVAL;
    std::vector<uint64_t> pack;
    try {
        pack.resize(n);
    } catch (const std::bad_alloc &) {
        return MTCP_GPU_ENOMEM;
    }
    gather = 0;
    for (uint32_t i = 0; i < n; ++i) pack[i] = gather, gather += pad16(req[i].len);
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    const RcvreadLayout l(n, gather, mg::read_work(n, max_id).bytes);
    Stage &s = ctx->stage[0];
    int rc = stage_pinned(ctx, s, l, 0, 0, dl);
    if (rc != MTCP_GPU_OK) return rc;
    Call hc(s, dl, {ctx, dl});
    hc.up(l.req(s), req, l.req.bytes);
    hc.up(l.pack(s), pack.data(), l.pack.bytes);
    if (hc.ok())
        hc.note(rcvread_launch(ctx, l.req(s), n, max_id, d_state, d_rbuf, d_tx, d_snd, d_arena, arena_bytes,
                               l.bytes(s), dst_bytes, gather, l.pack(s), l.rres(s), l.total(s), l.work(s), s.stream));
    const uint8_t *h = hc.down_pinned(s.d_buf + l.back_off, l.back_bytes());
    if ((rc = hc.finish()) != MTCP_GPU_OK) return rc;
    l.copy_out(h, {{rres, l.rres}, {total, l.total}});
    const uint8_t *bytes = h + (l.bytes.off - l.back_off);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t len = rres[i].copylen;
        // what the device checked, once more before host memory is written
        if (len && len <= req[i].len && req[i].dst_off <= dst_bytes && len <= dst_bytes - req[i].dst_off)
            memcpy(static_cast<uint8_t *>(dst) + req[i].dst_off, bytes + pack[i], len);
    }
    return MTCP_GPU_OK;
}

// ---- the batched application write into device send buffers ----
static_assert(sizeof(mtcp_gpu_sndwrite_req) == 32 && offsetof(mtcp_gpu_sndwrite_req, len) == 4 &&
              offsetof(mtcp_gpu_sndwrite_req, src_off) == 8 && offsetof(mtcp_gpu_sndwrite_req, flags) == 16 &&
              offsetof(mtcp_gpu_sndwrite_req, rsvd) == 20,
              "sndwrite_step.hpp reads the request as dwords; the claim kernels read its sid");
static_assert(sizeof(mtcp_gpu_sndwrite_res) == 16 && offsetof(mtcp_gpu_sndwrite_res, written) == 4 &&
              offsetof(mtcp_gpu_sndwrite_res, snd_wnd) == 8 && offsetof(mtcp_gpu_sndwrite_res, verdict) == 12 &&
              offsetof(mtcp_gpu_sndwrite_res, flags) == 13 && offsetof(mtcp_gpu_sndwrite_res, rsvd) == 14,
              "sndwrite_step.hpp writes the record as dwords");
static_assert(sizeof(mtcp_gpu_ack_state) == 128 && offsetof(mtcp_gpu_ack_state, snd_wnd) == 8 &&
              offsetof(mtcp_gpu_ack_state, sb_head_seq) == 64 && offsetof(mtcp_gpu_ack_state, sb_len) == 68 &&
              offsetof(mtcp_gpu_ack_state, sb_size) == 72 && offsetof(mtcp_gpu_ack_state, mss) == 76 &&
              offsetof(mtcp_gpu_ack_state, tcp_state) == 80 && offsetof(mtcp_gpu_ack_state, nrtx) == 84 &&
              offsetof(mtcp_gpu_ack_state, has_sndbuf) == 86 && sizeof(mtcp_gpu_datagen_state) == 16 &&
              offsetof(mtcp_gpu_datagen_state, sb_base_seq) == 8 && offsetof(mtcp_gpu_datagen_state, on_send_list) == 12,
              "write_step's dwords and sndwrite_plan_kernel's loads and stores");

namespace {

bool sndwrite_geom_ok(uint32_t n, uint32_t max_id) {
    return n <= MTCP_GPU_GROUP_MAX_PKTS && max_id <= MTCP_GPU_FLOWTAB_MAX_ID;
}

// what both forms ask of the device-resident arguments
bool sndwrite_mirrors_ok(const mtcp_gpu_ctx *ctx, uint32_t n, uint32_t max_id, const void *d_snd, const void *d_dtx,
                         const void *d_payload, uint64_t payload_bytes) {
    if (!ctx || !sndwrite_geom_ok(n, max_id) || (n && (!d_snd || !d_dtx || !d_payload))) return false;
    return !(((uintptr_t)d_snd & 127) || ((uintptr_t)d_dtx & 15) || ((uintptr_t)d_payload & 15) || (payload_bytes & 15));
}

bool sndwrite_dev_args_ok(const mtcp_gpu_ctx *ctx, const void *d_wreq, uint32_t n, uint32_t max_id, const void *d_snd,
                          const void *d_dtx, const void *d_src, uint64_t src_bytes, const void *d_payload,
                          uint64_t payload_bytes, const void *d_wres, const void *d_seg_sid, const void *d_seg_start,
                          const void *d_seg_stop, const void *d_nseg, const void *d_total, const void *d_work,
                          uint64_t work_bytes) {
    if (!sndwrite_mirrors_ok(ctx, n, max_id, d_snd, d_dtx, d_payload, payload_bytes)) return false;
    if (n && (!d_wreq || !d_src || !d_wres || !d_seg_sid || !d_seg_start || !d_seg_stop || !d_nseg || !d_total ||
              !d_work))
        return false;
    if (((uintptr_t)d_wreq & 15) || ((uintptr_t)d_src & 15) || (src_bytes & 15) || ((uintptr_t)d_wres & 15) ||
        ((uintptr_t)d_seg_sid & 3) || ((uintptr_t)d_seg_start & 3) || ((uintptr_t)d_seg_stop & 3) ||
        ((uintptr_t)d_nseg & 3) || ((uintptr_t)d_total & 7) || ((uintptr_t)d_work & 15))
        return false;
    return !n || work_bytes >= mg::read_work(n, max_id).bytes;
}

// The six launches; d_pack: the synchronous form's pack offsets, or nullptr.  d_src: the base the copy reads
// from, load_bytes of it; src_bytes: what BAD_REQ tests src_off + len against.
int sndwrite_launch(mtcp_gpu_ctx *ctx, const mtcp_gpu_sndwrite_req *d_wreq, uint32_t n, uint32_t max_id,
                    mtcp_gpu_ack_state *d_snd, mtcp_gpu_datagen_state *d_dtx, const void *d_src, uint64_t src_bytes,
                    uint64_t load_bytes, const uint64_t *d_pack, void *d_payload, uint64_t payload_bytes,
                    mtcp_gpu_sndwrite_res *d_wres, uint32_t *d_seg_sid, uint32_t *d_seg_start, uint32_t *d_seg_stop,
                    uint32_t *d_nseg, uint64_t *d_total, void *d_work, hipStream_t st) {
    const mg::ReadWork w = mg::read_work(n, max_id);                // the same claim words, prefixes and plan rows
    const mg::ReadParams C{n, max_id, 0, 0};
    const mg::WriteParams P{n, max_id, src_bytes, payload_bytes};
    uint8_t *work = static_cast<uint8_t *>(d_work);
    uint32_t *claim = reinterpret_cast<uint32_t *>(work + w.claim_off);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(work + w.cnt_off);
    uint32_t *part = reinterpret_cast<uint32_t *>(work + w.part_off);
    uint32_t *tot = reinterpret_cast<uint32_t *>(work + w.tot_off);
    uint4 *plan = reinterpret_cast<uint4 *>(work + w.plan_off);
    const uint4 *req = reinterpret_cast<const uint4 *>(d_wreq);
    const dim3 block(mg::kBlock), grid(w.nwg);
    hipLaunchKernelGGL(mg::rcvread_clear_kernel, grid, block, 0, st, req, C, claim, d_total);
    hipLaunchKernelGGL(mg::rcvread_claim_kernel, grid, block, 0, st, req, C, claim);
    hipLaunchKernelGGL(mg::sndwrite_plan_kernel, grid, block, 0, st, req, P, claim, reinterpret_cast<uint32_t *>(d_snd),
                       reinterpret_cast<uint32_t *>(d_dtx), d_pack, reinterpret_cast<uint4 *>(d_wres), d_seg_sid,
                       d_seg_start, d_seg_stop, d_nseg, d_total, cnt, part, plan);
    hipLaunchKernelGGL(mg::steer_scan_kernel, dim3(1), block, 0, st, part, w.nwg, tot);
    const uint32_t mgrid = (uint32_t)(((uint64_t)n + mg::kWavesPerBlock - 1) / mg::kWavesPerBlock);
    hipLaunchKernelGGL(mg::sndwrite_move_kernel, dim3(mgrid), block, 0, st, plan, n, (uint64_t)(uintptr_t)d_payload);
    // a wave per unit up to eight workgroups a CU; the grid walks what is beyond with its stride.  The units of
    // disjoint chunks: one per request for a ragged end, and the bytes that can be loaded and stored
    const uint64_t units = (uint64_t)n + std::min(load_bytes, payload_bytes) / mg::kWriteUnit;
    const uint64_t wgs = (units + mg::kWavesPerBlock - 1) / mg::kWavesPerBlock;
    const uint32_t cgrid = (uint32_t)std::min<uint64_t>(wgs, (uint64_t)ctx->num_cu * 8);
    hipLaunchKernelGGL(mg::sndwrite_copy_kernel, dim3(cgrid), block, 0, st, cnt, part, tot, w.nwg, plan,
                       (uint64_t)(uintptr_t)d_src, (uint64_t)(uintptr_t)d_payload);
    ctx->last_kernel = "sndwrite_copy_kernel";
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

}  // namespace

uint32_t mtcp_gpu_sndwrite_tile(void) { return mg::kWriteUnit; }

uint64_t mtcp_gpu_sndwrite_work_bytes(uint32_t n, uint32_t max_id) {
    if (!sndwrite_geom_ok(n, max_id)) return 0;
    return mg::read_work(n, max_id).bytes;
}

int mtcp_gpu_sndwrite_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_sndwrite_req *d_wreq, uint32_t n, uint32_t max_id,
                          mtcp_gpu_ack_state *d_snd, mtcp_gpu_datagen_state *d_dtx, const void *d_src,
                          uint64_t src_bytes, void *d_payload, uint64_t payload_bytes, mtcp_gpu_sndwrite_res *d_wres,
                          uint32_t *d_seg_sid, uint32_t *d_seg_start, uint32_t *d_seg_stop, uint32_t *d_nseg,
                          uint64_t *d_total, void *d_work, uint64_t work_bytes, void *stream) {
    if (!sndwrite_dev_args_ok(ctx, d_wreq, n, max_id, d_snd, d_dtx, d_src, src_bytes, d_payload, payload_bytes, d_wres,
                              d_seg_sid, d_seg_start, d_seg_stop, d_nseg, d_total, d_work, work_bytes))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    return sndwrite_launch(ctx, d_wreq, n, max_id, d_snd, d_dtx, d_src, src_bytes, src_bytes, nullptr, d_payload,
                           payload_bytes, d_wres, d_seg_sid, d_seg_start, d_seg_stop, d_nseg, d_total, d_work,
                           pick(ctx, stream));
}

int mtcp_gpu_write_send_dev(mtcp_gpu_ctx *ctx, const mtcp_gpu_sndwrite_req *d_wreq, uint32_t n, uint32_t max_id,
                            mtcp_gpu_ack_state *d_snd, mtcp_gpu_datagen_state *d_dtx, const void *d_src,
                            uint64_t src_bytes, void *d_payload, uint64_t payload_bytes, mtcp_gpu_sndwrite_res *d_wres,
                            uint32_t *d_seg_sid, uint32_t *d_seg_start, uint32_t *d_seg_stop, uint32_t *d_nseg,
                            uint64_t *d_wtotal, void *d_wwork, uint64_t wwork_bytes, const uint32_t *d_idx,
                            const mtcp_gpu_rcv_state *d_state, mtcp_gpu_ackgen_state *d_tx, uint32_t cur_ts,
                            const mtcp_gpu_tx_link *d_links, uint32_t n_links, void *d_buf, uint64_t buf_off,
                            uint64_t buf_len, uint32_t off_shift, uint32_t slot_bytes, uint16_t max_mss,
                            uint32_t flags, mtcp_gpu_tx_seg *d_seg, mtcp_gpu_desc *d_desc, uint32_t seg_cap,
                            mtcp_gpu_datagen_res *d_dres, uint64_t *d_total, uint8_t *d_status, void *d_work,
                            uint64_t work_bytes, void *stream) {
    // both calls' checks before either launches
    if (!sndwrite_dev_args_ok(ctx, d_wreq, n, max_id, d_snd, d_dtx, d_src, src_bytes, d_payload, payload_bytes, d_wres,
                              d_seg_sid, d_seg_start, d_seg_stop, d_nseg, d_wtotal, d_wwork, wwork_bytes) ||
        !datagen_dev_args_ok(ctx, nullptr, nullptr, n, max_id, d_idx, d_seg_sid, d_seg_start, d_nseg, d_seg_stop,
                             d_state, d_snd, d_tx, d_dtx, n_links, buf_off, off_shift, slot_bytes, d_seg, d_desc,
                             seg_cap, d_dres, d_total, d_work, work_bytes) ||
        !txbuild_args_ok(ctx, seg_cap, d_seg, d_payload, payload_bytes, d_links, n_links, d_buf, buf_len, d_desc,
                         off_shift, flags, d_status) ||
        ((uintptr_t)d_links & 3))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    const int rc = mtcp_gpu_sndwrite_dev(ctx, d_wreq, n, max_id, d_snd, d_dtx, d_src, src_bytes, d_payload,
                                         payload_bytes, d_wres, d_seg_sid, d_seg_start, d_seg_stop, d_nseg, d_wtotal,
                                         d_wwork, wwork_bytes, stream);
    if (rc != MTCP_GPU_OK) return rc;
    return mtcp_gpu_data_send_dev(ctx, nullptr, nullptr, n, max_id, d_idx, d_seg_sid, d_seg_start, d_nseg, d_seg_stop,
                                  d_state, d_snd, d_tx, d_dtx, cur_ts, d_payload, payload_bytes, d_links, n_links,
                                  d_buf, buf_off, buf_len, off_shift, slot_bytes, max_mss, flags, d_seg, d_desc,
                                  seg_cap, d_dres, d_total, d_status, d_work, work_bytes, stream);
}

int mtcp_gpu_sndwrite(mtcp_gpu_ctx *ctx, const mtcp_gpu_sndwrite_req *wreq, uint32_t n, uint32_t max_id,
                      mtcp_gpu_ack_state *d_snd, mtcp_gpu_datagen_state *d_dtx, const void *src, uint64_t src_bytes,
                      void *d_payload, uint64_t payload_bytes, mtcp_gpu_sndwrite_res *wres, uint32_t *seg_sid,
                      uint32_t *seg_start, uint32_t *seg_stop, uint32_t *nseg, uint64_t total[2]) {
    if (!sndwrite_mirrors_ok(ctx, n, max_id, d_snd, d_dtx, d_payload, payload_bytes) ||
        (n && (!wreq || !src || !wres || !seg_sid || !seg_start || !seg_stop || !nseg || !total)))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (n == 0) return MTCP_GPU_OK;
    // the packing: request i's bytes at pack[i] of the stage, len bytes each, 16 B aligned.  The bound is tested
    // before the table is allocated, and no exception leaves a C entry point
    uint64_t packed = 0;
    for (uint32_t i = 0; i < n; ++i)
        if ((packed += pad16(wreq[i].len)) > MTCP_GPU_SNDWRITE_HOST_MAX_BYTES) return MTCP_GPU_EINVAL;
    std::vector<uint64_t> pack;
    try {
        pack.resize(n);
    } catch (const std::bad_alloc &) {
        return MTCP_GPU_ENOMEM;
    }
    packed = 0;
    for (uint32_t i = 0; i < n; ++i) pack[i] = packed, packed += pad16(wreq[i].len);
    DeviceGuard dg(ctx->device);
    const Deadline dl(ctx->wait_us);
    const SndwriteLayout l(n, packed, mg::read_work(n, max_id).bytes);
    Stage &s = ctx->stage[0];
    int rc = stage_pinned(ctx, s, l, 0, 0, dl);
    if (rc != MTCP_GPU_OK) return rc;
    Call hc(s, dl, {ctx, dl});
    hc.up(l.req(s), wreq, l.req.bytes);
    hc.up(l.pack(s), pack.data(), l.pack.bytes);
    // the bytes of the requests whose range lies inside src: what the device tests too, before host memory is read
    for (uint32_t i = 0; i < n; ++i)
        if (wreq[i].len && wreq[i].src_off <= src_bytes && wreq[i].len <= src_bytes - wreq[i].src_off)
            hc.up(l.bytes(s) + pack[i], static_cast<const uint8_t *>(src) + wreq[i].src_off, wreq[i].len, true);
    if (hc.ok())
        hc.note(sndwrite_launch(ctx, l.req(s), n, max_id, d_snd, d_dtx, l.bytes(s), src_bytes, packed, l.pack(s),
                                d_payload, payload_bytes, l.wres(s), l.seg_sid(s), l.seg_start(s), l.seg_stop(s),
                                l.nseg(s), l.total(s), l.work(s), s.stream));
    return l.fetch(hc, s, {{wres, l.wres}, {seg_sid, l.seg_sid}, {seg_start, l.seg_start}, {seg_stop, l.seg_stop},
                           {nseg, l.nseg}, {total, l.total}});
}

// ---- RSS-friendly address pool -----------------------------
int mtcp_gpu_rss_queue_map_dev(mtcp_gpu_ctx *ctx, uint32_t saddr_base_h, uint32_t num_addr,
                               uint32_t daddr_h, uint16_t dport_h, int num_queues,
                               int endian_check, uint8_t *d_queue, void *stream) {
    if (!ctx || num_queues < 1 || (num_addr && !d_queue) || ((uintptr_t)d_queue & 3))
        return MTCP_GPU_EINVAL;
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (num_addr == 0) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    mg::PoolParams pp{};
    pp.rss_tables = ctx->d_rss_tables;
    pp.saddr_base_h = saddr_base_h;
    pp.daddr_h = daddr_h;
    pp.dport_h = dport_h;
    pp.nq = (uint32_t)num_queues;
    pp.endian = endian_check ? 1u : 0u;
    pp.total = (uint64_t)num_addr * mg::kPorts;
    // one tile of kQmapTile candidates per workgroup, up to 8 workgroups per
    // CU (the kernel walks further tiles grid-stride)
    const uint64_t tiles = (pp.total + mg::kQmapTile - 1) / mg::kQmapTile;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(tiles, (uint64_t)ctx->num_cu * 8);
    hipLaunchKernelGGL(mg::rss_queue_map_kernel, dim3(blocks), dim3(mg::kBlock), 0,
                       pick(ctx, stream), pp, d_queue);
    return HIP_OK(hipGetLastError()) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

int mtcp_gpu_addr_pool_search(mtcp_gpu_ctx *ctx, int core, int num_queues, uint32_t saddr_base,
                              int num_addr, uint32_t daddr, uint16_t dport, int endian_check,
                              mtcp_gpu_addr_entry *out, uint32_t max_out, uint32_t *n_found) {
    if (!ctx || num_queues < 1 || num_addr < 0 || !n_found || (max_out && !out))
        return MTCP_GPU_EINVAL;
    *n_found = 0;
    // addr_pool.c:129 computes num_entry in int: keep the product in range
    const uint64_t total = (uint64_t)num_addr * mg::kPorts;
    if (total > (uint64_t)INT32_MAX) return MTCP_GPU_EINVAL;
    const uint32_t num_entry = (uint32_t)((int)total / num_queues);
    if (ctx->abandoned) return MTCP_GPU_EIO;
    if (num_addr == 0 || core < 0 || core >= num_queues) return MTCP_GPU_OK;
    DeviceGuard dg(ctx->device);
    const uint32_t nb = (uint32_t)((total + mg::kPoolTile - 1) / mg::kPoolTile);
    const uint32_t limit = std::min(num_entry, max_out);
    const uint64_t qbytes = (total + 15) & ~15ull;
    uint8_t *d_mem = nullptr;
    const uint64_t out_off = (qbytes + 4ull * (nb + 1) + 7) & ~7ull;     // 8 B aligned entries
    const uint64_t bytes = out_off + 8ull * std::max(limit, 1u);
    if (!HIP_OK(mtcp_park::alloc(&d_mem, bytes, mtcp_park::kDevice))) return MTCP_GPU_ENOMEM;
    uint8_t *d_queue = d_mem;
    uint32_t *d_counts = reinterpret_cast<uint32_t *>(d_mem + qbytes);
    mtcp_gpu_addr_entry *d_out = reinterpret_cast<mtcp_gpu_addr_entry *>(d_mem + out_off);
    hipStream_t st = ctx->stream;
    const Deadline dl(ctx->wait_us);
    Stage &s0 = ctx->stage[0];                                             // its stream is st
    Call hc(s0, dl, {ctx, dl});
    const uint32_t saddr_base_h = __builtin_bswap32(saddr_base);           // addr_pool.c:150
    hc.note(mtcp_gpu_rss_queue_map_dev(ctx, saddr_base_h, (uint32_t)num_addr, __builtin_bswap32(daddr),
                                       (uint16_t)((dport >> 8) | (dport << 8)), num_queues, endian_check, d_queue,
                                       st));
    // what comes back comes down pinned (the count, then the entries),
    // copied out once its copy has finished
    if (hc.ok()) hc.note(stage_host(ctx, s0, 0, 8ull * std::max(limit, 1u), dl));
    if (hc.ok()) {
        hipLaunchKernelGGL(mg::pool_count_kernel, dim3(nb), dim3(mg::kBlock), 0, st, d_queue, total,
                           (uint32_t)core, d_counts);
        hipLaunchKernelGGL(mg::pool_scan_kernel, dim3(1), dim3(mg::kBlock), 0, st, d_counts, nb);
        if (limit)
            hipLaunchKernelGGL(mg::pool_emit_kernel, dim3(nb), dim3(mg::kBlock), 0, st, d_queue,
                               total, (uint32_t)core, d_counts, saddr_base_h, limit, d_out);
        if (!HIP_OK(hipGetLastError())) hc.note(MTCP_GPU_EIO);
    }
    const uint8_t *h_count = hc.down_pinned(d_counts + nb, sizeof(uint32_t));
    int rc = hc.finish();                                    // after a failure too: d_mem is released below
    if (rc == MTCP_GPU_OK) {
        uint32_t count;
        memcpy(&count, h_count, sizeof(count));
        const uint32_t kept = std::min(count, num_entry);
        const uint32_t copy = std::min(kept, max_out);
        const uint8_t *h_ent = hc.down_pinned(d_out, (size_t)copy * sizeof(mtcp_gpu_addr_entry));
        rc = hc.finish();
        if (rc == MTCP_GPU_OK) {
            if (copy) memcpy(out, h_ent, (size_t)copy * sizeof(mtcp_gpu_addr_entry));
            *n_found = kept;
        }
    }
    if (rc == MTCP_GPU_ETIMEDOUT) return rc;                 // abandoned: d_mem stays allocated
    if (!ctx->abandoned) mtcp_park::release(d_mem, bytes, mtcp_park::kDevice, !dl.bounded);
    return rc;
}

int mtcp_gpu_host_register(void *ptr, uint64_t len) {
    if (!ptr || !len) return MTCP_GPU_EINVAL;
    return HIP_OK(hipHostRegister(ptr, len, hipHostRegisterMapped)) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

int mtcp_gpu_host_unregister(void *ptr) {
    if (!ptr) return MTCP_GPU_EINVAL;
    return HIP_OK(hipHostUnregister(ptr)) ? MTCP_GPU_OK : MTCP_GPU_EIO;
}

}  // extern "C"
