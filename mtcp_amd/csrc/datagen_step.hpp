// datagen_step.hpp — WriteTCPDataList's body for one stream, the head of
// FlushTCPSendingBuffer and what SendTCPPacket leaves behind for data segments
// (mtcp/src/tcp_out.c:607-660, :357-449, :290, :301-306, :332, :346-350;
// mtcp/src/ip_out.c:139; mtcp/src/timer.c:37), with the rules of
// include/mtcp_gpu_datagen.h on top.  One text, __host__ __device__: the
// kernels (datagen_kernels.hpp) and tests/c/datagen_step_test.cpp (a plain g++
// build under the sanitizers, with a host loop over it) run it.  No HIP call
// is made here.
//
// Four pieces: the fold of one packet's flag word into on_send_list (and of 64
// of them given as masks, for the wave), the status of one stream in front of
// the flush, its burst for row f8, the commit from row f8's result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu_datagen.h"
#include "ackgen_step.hpp"   // AckGenTx, ackgen_bad: the d_tx record and its BAD rule

namespace mg {

// ---- the fold -------------------------------------------------------------------
// w: the last dword of an ACK record, flags | verdict << 16 | dup_acks << 24.
// RemoveFromSendList (tcp_in.c:453, tcp_out.c:891-892), then AddtoSendList
// (tcp_in.c:426, tcp_out.c:850-851): the add is applied last.
__host__ __device__ __forceinline__ uint32_t datagen_fold(uint32_t on, uint32_t w) {
    if (w & MTCP_GPU_ACK_SEND_LIST_REMOVE) on = 0;
    if (w & MTCP_GPU_ACK_FAST_RTX) on = 1;
    return on;
}

// The same over up to 64 packets in list order, packet i being bit i of the
// masks.  Last flag wins: the highest set position decides, the add where both
// masks have it.
__host__ __device__ __forceinline__ uint32_t datagen_fold_masks(uint32_t on, uint64_t add, uint64_t rm) {
    if (!(add | rm)) return on;
    return add > (rm & ~add) ? 1u : 0u;      // the highest set bit of add is at or above rm's
}

// ---- one stream's records ---------------------------------------------------------
// What the burst kernel loads of one stream.  dflags: on_send_list |
// on_control_list << 8 | rsvd << 16 (d_dtx dword 3); rstate: d_state dword 7
// (tcp_state in its low byte); mss2, bits, bits2: as ack_step.hpp's AckState
// (mss | eff_mss << 16; tcp_state | saw_timestamp << 8 | wscale_peer << 16 |
// dup_acks << 24; nrtx | on_rto << 8 | has_sndbuf << 16 | rsvd << 24).
struct DataGenIn {
    uint64_t sb_off;
    uint32_t sb_base_seq, dflags;
    AckGenTx tx;
    uint32_t rcv_nxt, rcv_wnd, ts_recent, rstate;
    uint32_t snd_nxt, snd_una, peer_wnd, cwnd, sb_head_seq, sb_len, sb_size, mss2, bits, bits2;
};

// TCP_SEQ_LT (tcp_in.h:37-41)
__host__ __device__ __forceinline__ bool datagen_seq_lt(uint32_t a, uint32_t b) { return (int32_t)(a - b) < 0; }

// The BAD test: d_dtx's own rule, d_tx by mtcp_gpu_ackgen.h's, d_snd by
// mtcp_gpu_ackwalk.h's (ack_step.hpp's test in front of every packet).
__host__ __device__ __forceinline__ bool datagen_bad(const DataGenIn &s, uint32_t n_links) {
    if ((s.dflags >> 16) || (s.dflags & 0xFFu) > 1u || ((s.dflags >> 8) & 0xFFu) > 1u) return true;
    if (ackgen_bad(s.tx, n_links)) return true;
    const uint32_t eff_mss = s.mss2 >> 16, wscale_peer = (s.bits >> 16) & 0xFFu;
    return (s.bits2 >> 24) != 0 || eff_mss == 0 || wscale_peer > 31u || s.sb_size > MTCP_GPU_ACK_MAX_SIZE ||
           s.sb_len > s.sb_size;
}

// The status in front of the flush, `on` being on_send_list after the fold.
// MTCP_GPU_DATAGEN_SENT stands for "the flush runs": the commit makes it
// BAD_BURST, SENT, WINDOW or NO_ROOM from row f8's result.
__host__ __device__ __forceinline__ uint32_t datagen_status(const DataGenIn &s, uint32_t n_links, uint32_t on,
                                                           bool host_tail) {
    if (datagen_bad(s, n_links)) return MTCP_GPU_DATAGEN_BAD;
    if (host_tail || (s.rstate & 0xFFu) != MTCP_GPU_RCV_ST_ESTABLISHED ||
        (s.bits & 0xFFu) != MTCP_GPU_ACK_ST_ESTABLISHED)
        return MTCP_GPU_DATAGEN_DEFERRED;
    if (!on) return MTCP_GPU_DATAGEN_IDLE;                                      // tcp_out.c:608
    if ((s.dflags >> 8) & 1u) return MTCP_GPU_DATAGEN_CONTROL_WAIT;             // tcp_out.c:614-617
    if (!((s.bits2 >> 16) & 0xFFu)) return MTCP_GPU_DATAGEN_NO_SNDBUF;          // tcp_out.c:369-373
    if (s.sb_len == 0) return MTCP_GPU_DATAGEN_EMPTY;                           // tcp_out.c:377-380
    if (datagen_seq_lt(s.snd_nxt, s.sb_head_seq)) return MTCP_GPU_DATAGEN_BEHIND_HEAD;   // tcp_out.c:387-394
    if (s.snd_nxt - s.sb_head_seq > s.sb_len || s.snd_nxt - s.snd_una > MTCP_GPU_DATAGEN_MAX_DIST ||
        s.snd_nxt - s.sb_base_seq > MTCP_GPU_DATAGEN_MAX_DIST ||
        s.sb_head_seq - s.sb_base_seq > MTCP_GPU_DATAGEN_MAX_DIST)
        return MTCP_GPU_DATAGEN_BAD_BURST;
    return MTCP_GPU_DATAGEN_SENT;
}

// rcv_wnd >> wscale_mine (tcp_out.c:298-301); the record is not BAD: the shift is below 32.
__host__ __device__ __forceinline__ uint32_t datagen_window32(const DataGenIn &s) {
    return s.rcv_wnd >> (s.tx.misc & 31u);
}

// The sixteen dwords of the stream's mtcp_gpu_tx_burst, its status being
// "the flush runs".
__host__ __device__ __forceinline__ void datagen_burst(const DataGenIn &s, uint32_t cur_ts, uint32_t out[16]) {
    const uint64_t po = s.sb_off + (uint64_t)(uint32_t)(s.snd_nxt - s.sb_base_seq);   // tcp_out.c:404-405
    const uint32_t window32 = datagen_window32(s);
    out[0] = (uint32_t)po, out[1] = (uint32_t)(po >> 32);
    out[2] = s.tx.saddr, out[3] = s.tx.daddr, out[4] = s.tx.ports;
    out[5] = s.snd_nxt;                                                          // tcp_out.c:385
    out[6] = s.rcv_nxt;                                                          // tcp_out.c:289
    out[7] = cur_ts, out[8] = s.ts_recent;                                       // tcp_out.c:118-122
    out[9] = s.sb_head_seq + s.sb_len - s.snd_nxt;                               // tcp_out.c:395
    out[10] = s.snd_nxt - s.snd_una;                                             // tcp_out.c:421
    out[11] = s.cwnd < s.peer_wnd ? s.cwnd : s.peer_wnd;                         // tcp_out.c:382
    out[12] = s.peer_wnd;                                                        // tcp_out.c:423
    out[13] = (window32 < 65535u ? window32 : 65535u) | (s.tx.id_cnt & 0xFFFFu) << 16;   // tcp_out.c:302, ip_out.c:139
    out[14] = (s.mss2 & 0xFFFFu) | ((s.tx.misc >> 8) & 0xFFu) << 16;             // tcp_out.c:360
    out[15] = 0;
}

// The burst of every other segment: len 0, which row f8 accepts as OK with no
// segment (the smallest mss it takes, link 0).
__host__ __device__ __forceinline__ void datagen_burst_void(uint32_t out[16]) {
    for (int i = 0; i < 16; ++i) out[i] = 0;
    out[14] = 13u;
}

// What the burst kernel parks for the commit, one dword a segment: status |
// on_send_list on entry << 8 | after the fold << 9 | (window32 == 0) << 10.
__host__ __device__ __forceinline__ uint32_t datagen_park(uint32_t status, uint32_t on_before, uint32_t on_fold,
                                                         bool win0) {
    return status | (on_before & 1u) << 8 | (on_fold & 1u) << 9 | (win0 ? 1u << 10 : 0u);
}

// ---- the commit -------------------------------------------------------------------
// What one stream's commit stores: each value with its own "store it" bit.
struct DataGenCommit {
    uint32_t res[4];            // the result record
    uint32_t snd_nxt;           // d_snd dword 0
    uint32_t ts_rto;            // d_snd dword 10, and on_rto = 1 (byte 85)
    uint32_t id_cnt, misc;      // d_tx dwords 3 and 4
    uint32_t ts_lastack_sent;   // d_tx dword 5
    uint32_t on_send_list;      // d_dtx byte 12
    bool st_snd_nxt, st_rto, st_id_cnt, st_misc, st_ts, st_on;
};

// park: the burst kernel's word; f8: row f8's result for the stream's burst
// (first_seg, n_seg, bytes, status | stop << 8); snd_nxt, rto, bits2: d_snd
// dwords 0, 9 and 21; id_cnt, misc, ts_lastack_sent: d_tx dwords 3-5 (read only
// where the status is past BAD).
__host__ __device__ __forceinline__ DataGenCommit datagen_commit(uint32_t park, const uint32_t f8[4], uint32_t snd_nxt,
                                                                 uint32_t rto, uint32_t bits2, uint32_t id_cnt,
                                                                 uint32_t misc, uint32_t ts_lastack_sent,
                                                                 uint32_t cur_ts) {
    DataGenCommit c{};
    uint32_t status = park & 0xFFu;
    const uint32_t on_before = (park >> 8) & 1u, on_fold = (park >> 9) & 1u, win0 = (park >> 10) & 1u;
    c.res[0] = f8[0];
    if (status <= MTCP_GPU_DATAGEN_BAD) {
        c.res[3] = status;
        return c;
    }
    uint32_t on = on_fold, flags = 0, e = 0, bytes = 0, stop = 0;
    int ret = -1;                                                               // < 0: the stream stays listed
    if (status == MTCP_GPU_DATAGEN_SENT) {
        if (f8[3] & 0xFFu) {
            status = MTCP_GPU_DATAGEN_BAD_BURST;
        } else {
            e = f8[1], bytes = f8[2], stop = (f8[3] >> 8) & 0xFFu;
            if (stop & MTCP_GPU_TXS_STOP_NO_ROOM) status = MTCP_GPU_DATAGEN_NO_ROOM, ret = -2;     // tcp_out.c:439-441
            else if (stop & MTCP_GPU_TXS_STOP_WINDOW) status = MTCP_GPU_DATAGEN_WINDOW, ret = -3;  // tcp_out.c:433
            else ret = (int)e;                                                  // tcp_out.c:443
            c.snd_nxt = snd_nxt + bytes, c.st_snd_nxt = true;                   // tcp_out.c:332
            uint32_t wack = (id_cnt >> 24) & 1u, nwa = (misc >> 24) & 1u, t = ts_lastack_sent;
            if (e) {
                c.ts_rto = cur_ts + rto, c.st_rto = true;                       // tcp_out.c:346
                if (!((bits2 >> 8) & 0xFFu)) flags |= MTCP_GPU_DATAGEN_RTO_ADD;  // timer.c:37
                t = cur_ts;                                                     // tcp_out.c:290
                c.ts_lastack_sent = cur_ts, c.st_ts = true;
                if (win0) nwa = 1, flags |= MTCP_GPU_DATAGEN_NEED_WND_ADV;      // tcp_out.c:304-306
            }
            if (status == MTCP_GPU_DATAGEN_WINDOW && (stop & MTCP_GPU_TXS_STOP_PEER_WINDOW) &&
                ((cur_ts - t) * 1000u) / 1000u > 500u)                          // tcp_out.c:429, tcp_in.h:44-50
                wack = 1, flags |= MTCP_GPU_DATAGEN_WACK_ENQUEUED;              // tcp_out.c:430, :931-933
            id_cnt = ((id_cnt + e) & 0xFFFFu) | (id_cnt & 0x00FF0000u) | wack << 24;   // ip_out.c:139
            misc = (misc & 0x00FFFFFFu) | nwa << 24;
            c.st_id_cnt = c.st_misc = true;
        }
    } else if (status == MTCP_GPU_DATAGEN_NO_SNDBUF || status == MTCP_GPU_DATAGEN_EMPTY ||
               status == MTCP_GPU_DATAGEN_BEHIND_HEAD) {
        ret = 0;
    }
    if (ret >= 0) {
        on = 0;                                                                 // tcp_out.c:639
        const uint32_t cnt = (id_cnt >> 16) & 0xFFu;
        if (cnt > 0) {                                                          // tcp_out.c:643-650
            const uint32_t left = (int)cnt > ret ? cnt - (uint32_t)ret : 0u;
            id_cnt = (id_cnt & 0xFF00FFFFu) | left << 16;
            c.st_id_cnt = true;
        }
    }
    c.id_cnt = id_cnt, c.misc = misc;
    c.on_send_list = on, c.st_on = on != on_before;
    flags |= (on_before ? MTCP_GPU_DATAGEN_ON_LIST_BEFORE : 0u) | (on ? MTCP_GPU_DATAGEN_ON_LIST_AFTER : 0u);
    c.res[1] = e, c.res[2] = bytes;
    c.res[3] = status | stop << 8 | flags << 16;
    return c;
}

}  // namespace mg
