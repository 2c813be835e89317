// stage_layout.hpp — where each host-memory call puts its pieces in stage 0's
// chunk buffer and what that asks of the pinned h_in / h_out.  Host-side C++,
// no HIP call, no kernel header: a workspace's size comes in as a number.
// tests/c/stage_layout_test.cpp checks every layout on the CPU.
#pragma once
#include <initializer_list>

#include "../../include/mtcp_gpu_rcvread.h"
#include "../../include/mtcp_gpu_rtosweep.h"   // and through it the records of every row before it
#include "../../include/mtcp_gpu_sndwrite.h"
#include "host_call.hpp"

namespace mtcp_host {

struct Region {
    uint64_t off = 0, bytes = 0;
};
template <class T>
struct Reg : Region {                           // a region of T; r(s): where it begins in stage s's chunk buffer
    T *operator()(const Stage &s) const { return reinterpret_cast<T *>(s.d_buf + off); }
};

// kIn: the region goes up (the next slot of h_in in a bounded call; kStreamed:
// written there with bounce_in).  kBack: part of the back piece, the
// contiguous span a bounded call brings down pinned in one D2H.
enum : unsigned { kIn = 1, kStreamed = 2, kBack = 4 };

// A result for the caller: the first `bytes` of back region r (all by default).
struct Out {
    void *dst;
    Region r;
    uint64_t bytes = ~0ull;
};

// Regions in the order they are put, each at the next multiple of its
// alignment (a power of two), the workspace last; the inputs in HostCall::in order.
struct StageLayout {
    Reg<uint8_t> work;
    uint64_t dev_bytes = 0;                     // the chunk buffer's
    uint64_t in_bytes = 0;                      // of h_in: each slot padded to 16 B but the last (HostCall::take's check)
    uint64_t in_next = 0, back_off = 0, back_end = 0;
    template <class T>
    void put(Reg<T> &r, uint64_t count, unsigned use = 0, uint64_t align = 16) {
        r.off = (dev_bytes + align - 1) & ~(align - 1), r.bytes = count * sizeof(T);
        dev_bytes = r.off + r.bytes;
        if (use & kIn) in(r.bytes, use & kStreamed);
        if ((use & kBack) && !back_end) back_off = r.off;     // the first of them: none is empty at offset 0
        if (use & kBack) back_end = dev_bytes;
    }
    // an input slot on its own: of what goes up elsewhere than into the chunk buffer
    void in(uint64_t bytes, bool streamed = false) {
        if (!bytes) return;                                   // HostCall::take: nothing to hold
        in_bytes = in_next + (streamed ? pad16(bytes) : bytes);
        in_next += pad16(bytes);
    }
    void end(uint64_t wbytes) { put(work, wbytes); }
    uint64_t back_bytes() const { return back_end - back_off; }
    // of h_out: the back piece, behind what comes down pinned before it (a tx call's image)
    uint64_t out_bytes(uint64_t first_bytes = 0) const { return pad16(first_bytes) + back_bytes(); }
    // results out of the back piece that came down pinned at `back`
    void copy_out(const uint8_t *back, std::initializer_list<Out> outs) const {
        for (const Out &o : outs)
            if (std::min(o.bytes, o.r.bytes)) memcpy(o.dst, back + (o.r.off - back_off), std::min(o.bytes, o.r.bytes));
    }
    // The back piece down pinned in one D2H and the round finished; the
    // results reach the caller only if that succeeded.
    template <class HC>
    int fetch(HC &hc, const Stage &s, std::initializer_list<Out> outs) const {
        const uint8_t *back = hc.down_pinned(s.d_buf + back_off, back_bytes());
        const int rc = hc.finish();
        if (rc == MTCP_GPU_OK) copy_out(back, outs);
        return rc;
    }
};

// A grouped batch's lists as inputs: idx[n], seg_sid[m], seg_start[m + 1], the
// clamped nseg; the generators put seg_stop[m] and ack_stop[m] behind them.
struct GroupLists {
    Reg<uint32_t> idx, seg_sid, seg_start, nseg, seg_stop, ack_stop;
    void put(StageLayout &l, uint32_t n, uint32_t m, unsigned in) {
        l.put(idx, n, in), l.put(seg_sid, m, in), l.put(seg_start, m + 1ull, in), l.put(nseg, 1, in);
    }
    // their upload; *m (the clamped nseg) lives until the call's finish()
    template <class HC>
    void up(HC &hc, const Stage &s, const uint32_t *idx_, const uint32_t *seg_sid_, const uint32_t *seg_start_,
            const uint32_t *m, const uint32_t *seg_stop_ = nullptr, const uint32_t *ack_stop_ = nullptr) const {
        hc.up(idx(s), idx_, idx.bytes);
        hc.up(seg_sid(s), seg_sid_, seg_sid.bytes);
        hc.up(seg_start(s), seg_start_, seg_start.bytes);
        hc.up(nseg(s), m, nseg.bytes);
        if (seg_stop_) hc.up(seg_stop(s), seg_stop_, seg_stop.bytes);
        if (ack_stop_) hc.up(ack_stop(s), ack_stop_, ack_stop.bytes);
    }
};

// mtcp_gpu_steer: the records (rec bytes each) go up into the stage's record buffer.
struct SteerLayout : StageLayout {
    Reg<uint32_t> idx, start;                   // adjacent: they come down together
    SteerLayout(uint32_t n, uint32_t Q, uint64_t rec, uint64_t wbytes) {
        in(n * rec);
        put(idx, n, kBack), put(start, Q + 2ull, kBack, 4);
        end(wbytes);
    }
};

// mtcp_gpu_group: nseg, alone in its 16 B, leads the outputs: a bounded call
// brings it down with the lists it bounds.
struct GroupLayout : StageLayout {
    Reg<uint32_t> sid, nseg, idx, seg_sid, seg_start;
    GroupLayout(uint32_t n, uint64_t wbytes) {
        put(sid, n, kIn), put(nseg, 1, kBack), put(idx, n, kBack);
        put(seg_sid, n, kBack, 4), put(seg_start, n + 1ull, kBack, 4);
        end(wbytes);
    }
};

// mtcp_gpu_rcvwalk and mtcp_gpu_ackwalk: the inputs (place[n]: the ACK walk's
// only), then what comes back: the states, a record per packet and the stops.
template <class State, class Rec>
struct WalkLayout : StageLayout {
    static_assert(sizeof(State) == 64 || sizeof(State) == 128, "a state is aligned to its size: the _dev entries' masks");
    Reg<mtcp_gpu_result> res;
    Reg<mtcp_gpu_tcpopt> opt;
    Reg<mtcp_gpu_rcv_place> place;
    GroupLists g;
    Reg<State> state;
    Reg<Rec> rec;
    Reg<uint32_t> stop;
    WalkLayout(uint32_t n, uint32_t max_id, uint32_t m, bool has_opt, bool has_place, uint64_t wbytes) {
        put(res, n, kIn), put(opt, has_opt ? n : 0, kIn), put(place, has_place ? n : 0, kIn), g.put(*this, n, m, kIn);
        put(state, max_id + 1ull, kIn | kBack, sizeof(State)), put(rec, n, kBack), put(stop, n, kBack);
        end(wbytes);
    }
};
using RcvwalkLayout = WalkLayout<mtcp_gpu_rcv_state, mtcp_gpu_rcv_place>;
using AckwalkLayout = WalkLayout<mtcp_gpu_ack_state, mtcp_gpu_ack_rec>;

// mtcp_gpu_ackgen (in_rec: place[n]) and mtcp_gpu_datagen (in_rec: ack[n], which
// comes with ack_stop or not at all; it alone has dtx).  An empty batch uploads
// nothing and has no streams.  The back piece begins at the first state written.
template <class In, class Res>
struct GenLayout : StageLayout {
    Reg<In> in_rec;
    GroupLists g;
    Reg<mtcp_gpu_ack_state> snd;
    Reg<mtcp_gpu_rcv_state> state;
    Reg<mtcp_gpu_ackgen_state> tx;
    Reg<mtcp_gpu_datagen_state> dtx;
    Reg<mtcp_gpu_tx_seg> seg;
    Reg<mtcp_gpu_desc> desc;
    Reg<Res> res;
    Reg<uint64_t> total;
    GenLayout(bool data, uint32_t n, uint32_t max_id, uint32_t m, bool ack_stop, uint32_t seg_cap, uint64_t wbytes) {
        const unsigned in = n ? kIn : 0;
        const uint64_t ids = n ? max_id + 1ull : 0;
        put(in_rec, n, data && !ack_stop ? 0 : in), g.put(*this, n, m, in);
        put(g.seg_stop, m, in), put(g.ack_stop, m, ack_stop ? in : 0);
        // ackgen: snd first, at its 128 B, so that state (64 B) and tx (32 B) follow with no padding
        if (data) put(state, ids, in, 128);
        put(snd, ids, data ? in | kBack : in, 128);
        if (!data) put(state, ids, in, 64);
        put(tx, ids, in | kBack, 32), put(dtx, data ? ids : 0, in | kBack);
        put(seg, seg_cap, kBack), put(desc, seg_cap, kBack), put(res, n, kBack), put(total, 2, kBack);
        end(wbytes);
    }
};
using AckgenLayout = GenLayout<mtcp_gpu_rcv_place, mtcp_gpu_ackgen_res>;
using DatagenLayout = GenLayout<mtcp_gpu_ack_rec, mtcp_gpu_datagen_res>;

// mtcp_gpu_rto_sweep: snd and dtx go up and come back, the sweep's lists behind them.
struct RtoLayout : StageLayout {
    Reg<mtcp_gpu_ack_state> snd;
    Reg<mtcp_gpu_datagen_state> dtx;
    Reg<mtcp_gpu_rto_rec> rto;
    Reg<uint32_t> seg_sid, seg_start, seg_stop, nseg;
    Reg<uint64_t> total;
    RtoLayout(uint32_t max_id, uint32_t cap, uint64_t wbytes) {
        put(snd, max_id + 1ull, kIn | kBack, 128), put(dtx, max_id + 1ull, kIn | kBack), put(rto, cap, kBack);
        put(seg_sid, cap, kBack), put(seg_start, cap + 1ull, kBack), put(seg_stop, cap, kBack);
        put(nseg, 1, kBack), put(total, 2, kBack);
        end(wbytes);
    }
};

// mtcp_gpu_rcvread: the requests and the gather's offsets go up; the records,
// the totals and the gathered bytes (gather_bytes of them) come back.
struct RcvreadLayout : StageLayout {
    Reg<mtcp_gpu_rcvread_req> req;
    Reg<uint64_t> pack, total;
    Reg<mtcp_gpu_rcvread_res> rres;
    Reg<uint8_t> bytes;
    RcvreadLayout(uint32_t n, uint64_t gather_bytes, uint64_t wbytes) {
        put(req, n, kIn), put(pack, n, kIn), put(rres, n, kBack), put(total, 2, kBack), put(bytes, gather_bytes, kBack);
        end(wbytes);
    }
};

// mtcp_gpu_sndwrite: the requests, the pack offsets and the packed bytes
// (pack_bytes of them, a slot per request) go up; the records, the table and
// the totals come back.
struct SndwriteLayout : StageLayout {
    Reg<mtcp_gpu_sndwrite_req> req;
    Reg<uint64_t> pack, total;
    Reg<uint8_t> bytes;
    Reg<mtcp_gpu_sndwrite_res> wres;
    Reg<uint32_t> seg_sid, seg_start, seg_stop, nseg;
    SndwriteLayout(uint32_t n, uint64_t pack_bytes, uint64_t wbytes) {
        put(req, n, kIn), put(pack, n, kIn), put(bytes, pack_bytes, kIn | kStreamed);
        put(wres, n, kBack), put(seg_sid, n, kBack), put(seg_start, n + 1ull, kBack), put(seg_stop, n, kBack);
        put(nseg, 1, kBack), put(total, 2, kBack);
        end(wbytes);
    }
};

// mtcp_gpu_tx_build (four arguments) and mtcp_gpu_tx_send: the frames' image
// leads; it is never uploaded and comes down pinned, whole, before the back piece.
struct TxLayout : StageLayout {
    Reg<uint8_t> image, payload, status;
    Reg<mtcp_gpu_tx_burst> burst;
    Reg<mtcp_gpu_tx_link> links;
    Reg<mtcp_gpu_tx_seg> seg;
    Reg<mtcp_gpu_desc> desc;
    Reg<mtcp_gpu_tx_burst_result> res;
    Reg<uint64_t> total;
    TxLayout(uint32_t n, uint32_t n_links, uint64_t payload_bytes, uint64_t buf_len) {
        put(image, buf_len), put(payload, payload_bytes, kIn | kStreamed), put(seg, n, kIn), put(links, n_links, kIn);
        in(n * sizeof(mtcp_gpu_desc));                        // they go up into the stage's descriptor buffer
        put(status, n, kBack);
        end(0);
    }
    TxLayout(uint32_t n_burst, uint32_t n_links, uint64_t payload_bytes, uint64_t buf_len, uint32_t seg_cap,
             uint64_t wbytes) {
        put(image, buf_len), put(payload, payload_bytes, kIn | kStreamed), put(burst, n_burst, kIn);
        put(links, n_links, kIn), put(seg, seg_cap), put(desc, seg_cap, kBack), put(status, seg_cap, kBack);
        put(res, n_burst, kBack), put(total, 2, kBack);
        end(wbytes);
    }
};

}  // namespace mtcp_host
