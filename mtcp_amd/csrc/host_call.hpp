// host_call.hpp — the staging of the host-memory calls and the one place
// that knows their wait-limit contract (include/mtcp_gpu.h).
// Host-side C++: no HIP call is made here except through a backend.
//
// A context without a wait limit (unbounded): a call's copies read and write
// the caller's memory directly.  With one (bounded): the call reads and
// writes the caller's memory only on the calling thread; every copy it queues
// goes through the stage's pinned h_in / h_out, a failed enqueue still drains
// the stream within the deadline, nothing reaches the caller unless the last
// drain succeeded, and past the deadline the context is abandoned (the copies
// given up on may still run, into the pinned buffers only).
//
// Stage holds a pipeline stage's buffers and the copy-outs a bounded call
// still owes the caller; HostCall is a synchronous call on one stage.
// tests/c/host_call_test.cpp runs both on the CPU with a recording backend.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/mtcp_gpu.h"
#include "../../include/mtcp_gpu_tcpopt.h"
#include "host_copy.hpp"
#include "wait.hpp"

namespace mtcp_host {

constexpr int kStages = 3;                       // H2D | kernel | D2H overlap
constexpr uint64_t kStageBytes = 64ull << 20;    // chunk bytes per pipeline stage
constexpr uint32_t kStagePkts = 1u << 16;        // descriptors per pipeline stage
inline uint64_t pad16(uint64_t v) { return (v + 15) & ~15ull; }

// What a bounded call still owes the caller once the stage's stream has
// drained: `bytes` from the pinned `src` to the caller's `dst`.
struct Pending {
    void *dst;
    const void *src;
    uint64_t bytes;
};
constexpr uint32_t kMaxPending = 2;              // an rx batch: its records and its option records

// One pipeline stage of the host-memory calls.  Stage 0 runs on the
// context's own stream (one stream per mTCP thread: an io_module's rxqs, its
// tx fills and every host call of a batch that fits one stage share it);
// stages 1 and 2 get streams of their own only when a call spans more than
// one stage (a chunk above kStageBytes), to overlap H2D, kernel and D2H.
struct Stage {
    uint8_t *d_buf = nullptr;
    mtcp_gpu_desc *d_desc = nullptr;
    mtcp_gpu_result *d_out = nullptr;
    uint64_t buf_cap = 0;
    uint32_t pkt_cap = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // bounded calls (a context wait limit): pinned bounce buffers, so that
    // no copy the call gives up on can read or write the caller's memory
    uint8_t *h_in = nullptr;                    // caller data -> H2D
    uint64_t h_in_cap = 0;
    uint8_t *h_out = nullptr;                   // D2H -> caller data
    uint64_t h_out_cap = 0;
    Pending pend[kMaxPending];                  // of this stage's batch, not yet copied out
    uint32_t npend = 0;
    // mtcp_gpu_rx_chunk_opts only: the batch's option records (kStagePkts of
    // them, allocated by the first such call) and their bounce buffer
    mtcp_gpu_tcpopt *d_opt = nullptr;
    mtcp_gpu_tcpopt *h_opt = nullptr;
};

// Owe the caller `bytes` at dst from the stage's pinned src (false: the list is full).
inline bool stage_pend(Stage &s, void *dst, const void *src, uint64_t bytes) {
    if (s.npend == kMaxPending) return false;
    s.pend[s.npend++] = Pending{dst, src, bytes};
    return true;
}

// The stage's stream has drained: what it owes reaches the caller.
inline void stage_copy_out(Stage &s) {
    for (uint32_t i = 0; i < s.npend; ++i)
        if (s.pend[i].bytes) memcpy(s.pend[i].dst, s.pend[i].src, s.pend[i].bytes);
    s.npend = 0;
}

// The call failed or gave up: nothing of it reaches the caller.
inline void stage_drop(Stage &s) { s.npend = 0; }

// A bounded call's copy of caller memory into a bounce buffer (16 B aligned
// destination, written up to the next 16 B; streaming stores: the DMA engine
// reads it next, not a core)
inline void bounce_in(uint8_t *dst, const void *src, uint64_t len) {
    const uint8_t *p = static_cast<const uint8_t *>(src);
    constexpr uint64_t kPiece = 1u << 30;
    for (uint64_t o = 0; o < len; o += kPiece)
        stage_copy(dst + o, p + o, (uint32_t)std::min(kPiece, len - o));
    stage_fence();
}

// A synchronous host call on one stage.  The caller has reserved the stage
// (device buffers, and h_in / h_out for what a bounded call bounces and for
// what comes down pinned); the slots of h_in and h_out are handed out here,
// in call order, each 16 B aligned.  The first failure is remembered: every
// later copy is a no-op and finish() answers it.
//
// Backend: bool copy(dst, src, bytes, up) queues one copy on the stage's
// stream (hipMemcpyAsync); int drain(rc) drains it within the deadline and
// answers rc, the drain's error if rc was OK, or MTCP_GPU_ETIMEDOUT (the
// context abandoned).
template <class Backend>
class HostCall {
public:
    HostCall(Stage &s, const mtcp_wait::Deadline &dl, Backend be) : s_(s), bounded_(dl.bounded), be_(be) {}

    bool bounded() const { return bounded_; }
    bool ok() const { return rc_ == MTCP_GPU_OK; }
    // the result of a step between the copies (a launch)
    void note(int rc) { rc_ = ok() ? rc : rc_; }

    // Where a queued copy may read the caller's `bytes` at host: there
    // (unbounded), or their copy in the next slot of h_in (bounded; streamed:
    // with bounce_in, for a chunk or a payload, else memcpy).
    const void *in(const void *host, uint64_t bytes, bool streamed = false) {
        if (!bounded_) return host;
        uint8_t *slot = take(s_.h_in, s_.h_in_cap, in_off_, bytes, streamed ? pad16(bytes) : bytes);
        if (!slot) return nullptr;
        if (streamed) bounce_in(slot, host, bytes);
        else if (bytes) memcpy(slot, host, bytes);
        return slot;
    }
    // One copy between library-owned host memory and the device.
    void h2d(void *dev, const void *src, uint64_t bytes) { copy(dev, src, bytes, true); }
    void d2h(void *dst, const void *dev, uint64_t bytes) { copy(dst, dev, bytes, false); }

    // The caller's input to the device.
    void up(void *dev, const void *host, uint64_t bytes, bool streamed = false) {
        h2d(dev, in(host, bytes, streamed), bytes);
    }
    // Two inputs to adjacent device ranges: their slots are adjacent too when
    // a_bytes is a multiple of 16, and a bounded call sends them in one H2D.
    void up2(void *dev, const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
        const void *pa = in(a, a_bytes), *pb = in(b, b_bytes);
        if (bounded_ && a_bytes % 16 == 0) return h2d(dev, pa, a_bytes + b_bytes);
        h2d(dev, pa, a_bytes);
        h2d(static_cast<uint8_t *>(dev) + a_bytes, pb, b_bytes);
    }
    // A result to the caller: straight there (unbounded), or into the next
    // slot of h_out and from there at finish() (bounded).
    void down(void *host, const void *dev, uint64_t bytes) { down2(host, dev, bytes, nullptr, 0); }
    // Two results from adjacent device ranges: one D2H when bounded.
    void down2(void *a, const void *dev, uint64_t a_bytes, void *b, uint64_t b_bytes) {
        if (!bounded_) {
            d2h(a, dev, a_bytes);
            return d2h(b, static_cast<const uint8_t *>(dev) + a_bytes, b_bytes);
        }
        const uint8_t *slot = down_pinned(dev, a_bytes + b_bytes);
        if (ok() && !(stage_pend(s_, a, slot, a_bytes) && (!b_bytes || stage_pend(s_, b, slot + a_bytes, b_bytes))))
            rc_ = MTCP_GPU_EIO;
    }
    // A result the call works on itself, into the next slot of h_out in
    // either mode: readable there once finish() answered MTCP_GPU_OK.
    const uint8_t *down_pinned(const void *dev, uint64_t bytes) {
        uint8_t *slot = take(s_.h_out, s_.h_out_cap, out_off_, bytes, bytes);
        if (slot) d2h(slot, dev, bytes);
        return slot;
    }

    // The end of a round (a call may have several: a count first, then a
    // count-sized piece): the stream drained, also after a failed enqueue; the
    // caller gets what it is owed only if all went well.  The slots start over.
    int finish() {
        if (rc_ == MTCP_GPU_ETIMEDOUT) return rc_;             // abandoned: no further wait
        rc_ = be_.drain(rc_);
        ok() ? stage_copy_out(s_) : stage_drop(s_);
        in_off_ = out_off_ = 0;
        return rc_;
    }

private:
    // the next slot of a pinned buffer; one that would pass its end is
    // refused (MTCP_GPU_EIO) and never written
    uint8_t *take(uint8_t *base, uint64_t cap, uint64_t &off, uint64_t bytes, uint64_t written) {
        if (!ok()) return nullptr;
        if (!bytes) return base + std::min(off, cap);         // nothing to hold
        if (off > cap || written > cap - off) {
            rc_ = MTCP_GPU_EIO;
            return nullptr;
        }
        uint8_t *slot = base + off;
        off += pad16(bytes);
        return slot;
    }
    void copy(void *dst, const void *src, uint64_t bytes, bool up) {
        if (ok() && bytes && !be_.copy(dst, src, bytes, up)) rc_ = MTCP_GPU_EIO;
    }

    Stage &s_;
    const bool bounded_;
    Backend be_;
    int rc_ = MTCP_GPU_OK;
    uint64_t in_off_ = 0, out_off_ = 0;
};

}  // namespace mtcp_host
