// tcpopt_kernels.hpp — gfx950 kernel of SURVEY §8 row f5: the two option
// walks of the reference's rx path, per packet of an rx batch:
//
//   ParseTCPTimestamp (mtcp/src/tcp_util.c:61-92; tcp_in.c:109) -> ts_val, ts_ref
//   ParseTCPOptions   (mtcp/src/tcp_util.c:14-59; tcp_in.c:72, :88)
//                                               -> mss, wscale, sack_permit, ts_recent
//
// One lane per packet.  The record (verdict, ihl_doff, tcp_flags) and the
// descriptor loads are coalesced; only a TCP_OK frame with doff > 5 costs a
// frame access: the aligned 16 B pieces that hold its option bytes and the
// up to 9 bytes behind them the reference may read (the length byte at index
// len, a timestamp ending at len + 8), at most four, and only pieces that
// hold at least one byte of the frame.  A lane parks its pieces in LDS, one
// column per lane (dword k of lane t at k * kBlock + t: every lane of a wave
// on its own bank whatever k the walks are at), and the byte walks index that
// column: a walk over a register array indexed at run time would go to
// scratch.  No lane reads another's column, so there is no barrier.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu_tcpopt.h"
#include "rx_kernels.hpp"

namespace mg {

constexpr int kOptMaxLen = 40;                      // 4 * 15 - 20
constexpr int kOptTail = 9;                         // bytes behind the options a walk may read
constexpr int kOptPieces = 4;                       // 14 + 40 + 9 = 63 bytes at most
constexpr int kOptDwords = 4 * kOptPieces;

struct OptParams {
    const uint8_t *buf;            // chunk base (chunk mode), 16 B aligned
    uint64_t buf_len;              // descriptor bound, as KParams
    int64_t base_sub;              // subtracted from every descriptor byte offset
    const mtcp_gpu_desc *desc;
    const uint8_t *const *ptrs;    // pointer mode
    const uint16_t *lens;
    uint32_t n;
    uint32_t off_shift;
    const void *res;               // the rx records: 40 B, or 16 B (CMP)
    uint4 *opt;                    // mtcp_gpu_tcpopt[n]
};

// The packed record {ts_val, ts_ref, ts_recent, mss | wscale << 16 | flags << 24}
// of one frame whose option bytes start at byte `o` of the lane's LDS column
// `col` (stride kBlock dwords).  len = 4*doff - 20 > 0; avail = bytes from
// the first option byte to the frame's end: a read at index >= avail makes
// the walk unpinned.  Every read is below min(avail, len + kOptTail).
__device__ __forceinline__ uint4 tcpopt_walks(const uint32_t *col, uint32_t o, int len, int avail,
                                              bool ts_walk, bool syn_walk) {
    auto rd = [&](int i) -> uint32_t {
        const uint32_t pos = o + (uint32_t)i;
        return (col[(pos >> 2) * kBlock] >> (8 * (pos & 3))) & 0xFFu;
    };
    auto rd32 = [&](int i) -> uint32_t {             // ntohl(*(uint32_t *)(tcpopt + i))
        return (rd(i) << 24) | (rd(i + 1) << 16) | (rd(i + 2) << 8) | rd(i + 3);
    };
    uint32_t ts_val = 0, ts_ref = 0, ts_recent = 0, mss = 0, wscale = 0, flags = 0;
    // every iteration of either walk moves at least one byte forward, except
    // the reference's endless one (a skipped option of length 0), which ends
    // the walk here: kOptMaxLen iterations cover any walk
    if (ts_walk) {                                   // tcp_util.c:68-91
        int i = 0;
        bool unpinned = false;
        for (int it = 0; it < kOptMaxLen && i < len; ++it) {
            if (i >= avail) { unpinned = true; break; }
            const uint32_t opt = rd(i++);
            if (opt == 0) break;                     // TCP_OPT_END
            if (opt == 1) continue;                  // TCP_OPT_NOP
            if (i >= avail) { unpinned = true; break; }
            const uint32_t optlen = rd(i++);
            if (i + (int)optlen - 2 > len) break;
            if (opt == 8) {                          // the first timestamp wins
                if (i + 8 > avail) { unpinned = true; break; }
                ts_val = rd32(i);
                ts_ref = rd32(i + 4);
                flags |= MTCP_GPU_TCPOPT_TS_FOUND;
                break;
            }
            if (optlen == 0) { unpinned = true; break; }   // i += -2: the same byte again
            i += (int)optlen - 2;
        }
        if (unpinned) flags |= MTCP_GPU_TCPOPT_TS_UNPINNED;
    }
    if (syn_walk) {                                  // tcp_util.c:21-58
        int i = 0;
        bool unpinned = false;
        uint32_t f = 0;
        for (int it = 0; it < kOptMaxLen && i < len; ++it) {
            if (i >= avail) { unpinned = true; break; }
            const uint32_t opt = rd(i++);
            if (opt == 0) break;
            if (opt == 1) continue;
            if (i >= avail) { unpinned = true; break; }
            const uint32_t optlen = rd(i++);
            if (i + (int)optlen - 2 > len) break;
            if (opt == 2) {                          // two bytes, whatever optlen says
                if (i + 2 > avail) { unpinned = true; break; }
                mss = (rd(i) << 8) + rd(i + 1);
                i += 2;
                f |= MTCP_GPU_TCPOPT_MSS;
            } else if (opt == 3) {
                if (i + 1 > avail) { unpinned = true; break; }
                wscale = rd(i);
                i += 1;
                f |= MTCP_GPU_TCPOPT_WSCALE;
            } else if (opt == 4) {
                f |= MTCP_GPU_TCPOPT_SACK_PERMIT;
            } else if (opt == 8) {                   // reads ts_val only, skips both
                if (i + 4 > avail) { unpinned = true; break; }
                ts_recent = rd32(i);
                i += 8;
                f |= MTCP_GPU_TCPOPT_SAW_TIMESTAMP;
            } else {
                if (optlen == 0) { unpinned = true; break; }
                i += (int)optlen - 2;
            }
        }
        if (unpinned) {
            ts_recent = mss = wscale = 0;
            flags |= MTCP_GPU_TCPOPT_SYN_UNPINNED;
        } else {
            flags |= f;
        }
    }
    return make_uint4(ts_val, ts_ref, ts_recent, mss | (wscale << 16) | (flags << 24));
}

// PTRS: a pointer burst instead of chunk + descriptors.  CMP: 16 B rx records.
template <bool PTRS, bool CMP>
__global__ __launch_bounds__(kBlock) void tcpopt_kernel(OptParams p) {
    __shared__ uint32_t win[kOptDwords * kBlock];    // 16 KiB: one column per lane
    uint32_t *col = win + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < p.n; i += stride) {
        // verdict, ihl | doff << 4, tcp_flags of the rx record
        uint32_t verdict, ihl_doff, tcp_flags;
        if constexpr (CMP) {
            const uint32_t w = reinterpret_cast<const uint32_t *>(p.res)[4 * i + 3];
            ihl_doff = w & 0xFFu, tcp_flags = (w >> 8) & 0xFFu, verdict = (w >> 16) & 0xFFu;
        } else {
            const uint2 w = reinterpret_cast<const uint2 *>(p.res)[5 * i + 4];   // bytes 32..39
            ihl_doff = (w.x >> 16) & 0xFFu, tcp_flags = w.x >> 24, verdict = w.y & 0xFFu;
        }
        // the frame, bounds-checked as rx does (rx_kernels.hpp)
        uint64_t fp = 0;
        uint32_t L = 0;
        bool ok = false;
        if constexpr (PTRS) {
            fp = (uint64_t)p.ptrs[i];
            L = p.lens[i];
            ok = fp != 0 && (fp & 1) == 0;
        } else {
            const uint2 d = reinterpret_cast<const uint2 *>(p.desc)[i];
            L = d.y & 0xFFFFu;
            const int64_t pos = (int64_t)((uint64_t)d.x << p.off_shift) - p.base_sub;
            ok = pos >= 0 && (pos & 1) == 0 && (uint64_t)pos + L <= p.buf_len;
            fp = (uint64_t)p.buf + (uint64_t)pos;
        }
        const int len = 4 * (int)(ihl_doff >> 4) - 20;
        const bool ts_walk = !(tcp_flags & 0x04u), syn_walk = (tcp_flags & 0x02u) != 0;
        uint4 rec = make_uint4(0, 0, 0, 0);
        if (ok && verdict == MTCP_GPU_V_TCP_OK && len > 0 && (ts_walk || syn_walk)) {
            const uint32_t first = 34u + 4u * (ihl_doff & 15u);      // the first option byte
            const int avail = (int)L - (int)first;                   // bytes up to the frame's end
            const uint64_t a = fp + first;
            const uint32_t o = (uint32_t)a & 15u;
            const int need = min(len + kOptTail, avail);
            const int pieces = need > 0 ? (int)((o + (uint32_t)need + 15u) >> 4) : 0;
            // every piece's load is issued before the first one is parked
            v4u v[kOptPieces];
#pragma unroll
            for (int c = 0; c < kOptPieces; ++c)
                if (c < pieces) v[c] = gload_nt((a & ~15ull) + 16ull * c);   // holds a byte of the frame
#pragma unroll
            for (int c = 0; c < kOptPieces; ++c) {
                if (c < pieces) {
                    col[(4 * c + 0) * kBlock] = v[c].x;
                    col[(4 * c + 1) * kBlock] = v[c].y;
                    col[(4 * c + 2) * kBlock] = v[c].z;
                    col[(4 * c + 3) * kBlock] = v[c].w;
                }
            }
            rec = tcpopt_walks(col, o, len, need, ts_walk, syn_walk);
        }
        p.opt[i] = rec;
    }
}

}  // namespace mg
