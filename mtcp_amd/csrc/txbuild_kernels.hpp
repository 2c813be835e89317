// txbuild_kernels.hpp — gfx950 kernels that build tx frames from segment
// records: what SendTCPPacket / SendTCPPacketStandalone
// (mtcp/src/tcp_out.c:135-354) do per segment with IPOutput* (ip_out.c:35-167)
// and EthernetOutput (eth_out.c:35-80): 54 B of headers, 12 or 20 B of
// options, the payload memcpy (tcp_out.c:195, :314) and the sum over every
// byte just copied (tcp_out.c:208, :327), in one pass.
//
// Work decomposition: a group of G lanes per segment (G = 64: a wave, 1 KiB
// of frame per pass, for jumbo payloads; G = 32: half a wave, whose three
// passes an MSS frame fills; G = 16: a DPP row; G = 8: eight lanes, one pass
// for the five or six chunks of an ACK-sized segment, for batches of those,
// which are record-bound; dispatch.hpp txbuild_group).  The frame
// is cut on the absolute 16 B grid of the destination; lane t of the group
// takes chunks t, t + G, ...
//   - a chunk's payload bytes come from two aligned 16 B source loads and a
//     byte funnel shift (the source address is arbitrary, the shift is the
//     same for every chunk of a segment); a source block is loaded only where
//     it overlaps the segment's payload, so nothing outside
//     [payload_off, payload_off + payload_len) is touched;
//   - v_sad_u16 adds the 16-bit halves of the shifted dwords: the payload
//     begins at an even frame offset and the frame at an even address, so
//     these are the reference's little-endian words whatever the source
//     alignment; bytes outside the payload are masked to zero first;
//   - chunks past the headers are stored at once, one aligned 16 B store
//     each (dword, short and byte stores only in the frame's first and last
//     chunk); the lanes that own the header chunks (at most six, in pass 0)
//     hold their payload bytes until the group's sum is reduced, since the TCP
//     check sits at frame byte 50, ahead of the payload;
//   - lane k of the group forms header dwords k, W + k, ... (W = min(G, 16)); the TCP header's and
//     the pseudo header's words join the sum there, a DPP row reduction (and
//     shuffles across the rows of a wider group) gives the total, one fold
//     (SURVEY §8 a2') gives the check, and the header lanes fetch their
//     dwords by shuffle.
// Each payload byte is loaded from HBM once (the second load of a lane is
// its neighbour's first), each frame byte is stored once, d_buf is never read.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtcp_gpu_txbuild.h"
#include "rx_kernels.hpp"

namespace mg {

struct TxBuildParams {
    const mtcp_gpu_tx_seg *seg;
    const uint8_t *payload;
    uint64_t payload_bytes;
    const mtcp_gpu_tx_link *links;
    uint32_t n_links;
    uint32_t n;
    uint8_t *buf;
    uint64_t buf_len;
    const mtcp_gpu_desc *desc;
    uint32_t off_shift;
    uint32_t max_mss;
    uint32_t no_csum;
    uint8_t *status;
};

typedef __attribute__((address_space(1))) v4u gsv4u;
typedef __attribute__((address_space(1))) uint32_t gsu32;
typedef __attribute__((address_space(1))) uint16_t gsu16;
typedef __attribute__((address_space(1))) uint8_t gsu8;
typedef __attribute__((address_space(1))) const uint32_t glu32;
typedef unsigned int v2u __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) const v2u glv2u;

__device__ __forceinline__ uint32_t gload32(uint64_t a) { return *reinterpret_cast<glu32 *>(a); }
__device__ __forceinline__ v2u gload64(uint64_t a) { return *reinterpret_cast<glv2u *>(a); }

// bytes [0, k) of a dword, k in 0..4
__device__ __forceinline__ uint32_t low_bytes(int k) {
    return k >= 4 ? 0xFFFFFFFFu : k <= 0 ? 0u : ((1u << (8 * k)) - 1u);
}
// bytes [lo, hi) of the dword that starts at frame byte b0, for the frame
// byte range [from, to)
__device__ __forceinline__ uint32_t byte_mask(int b0, int from, int to) {
    return low_bytes(to - b0) & ~low_bytes(from - b0);
}

// Stores bytes [lo, hi) of dword v at the 4 B aligned address a; lo is even.
__device__ __forceinline__ void store_part(uint64_t a, uint32_t v, int lo, int hi) {
    if (lo <= 0 && hi >= 4) {
        *reinterpret_cast<gsu32 *>(a) = v;
        return;
    }
    if (lo <= 0 && hi >= 2) *reinterpret_cast<gsu16 *>(a) = (uint16_t)v;
    if (lo <= 0 && hi == 1) *reinterpret_cast<gsu8 *>(a) = (uint8_t)v;
    if (lo <= 2 && hi >= 4) *reinterpret_cast<gsu16 *>(a + 2) = (uint16_t)(v >> 16);
    if (lo <= 2 && hi == 3) *reinterpret_cast<gsu8 *>(a + 2) = (uint8_t)(v >> 16);
}

// One segment's geometry and fields, the same in every lane of its group.
struct TxSeg {
    uint32_t status;
    uint64_t dst;        // frame byte 0 (even)
    uint64_t src;        // payload byte 0 (any alignment)
    int a;               // dst & 15
    int H;               // 54 + optlen: frame byte of payload byte 0
    int L;               // frame length
    uint32_t plen;
};

// Header dword k (frame bytes 4k .. 4k+3, little-endian) with both check
// fields as given (eth_out.c:72-77, ip_out.c:66-76, tcp_out.c:160-192,
// :79-122).  Dwords past the headers' end are zero there.
struct TxHdr {
    uint32_t l0, l1, l2;       // the link entry: dst[6] src[6]
    uint32_t saddr, daddr, ports;
    uint32_t seq_be, ack_be;   // as in memory
    uint32_t ver_len;          // tot_len, ip_id: as in memory
    uint32_t off_flags;        // frame bytes 46, 47
    uint32_t win_be;
    uint32_t o[5];             // option dwords, zero past optlen
};

__device__ __forceinline__ uint32_t tx_hdr_dword(const TxHdr &h, int k, uint32_t ip_check, uint32_t tcp_check) {
    uint32_t v = 0;
    v = k == 0 ? h.l0 : v;
    v = k == 1 ? h.l1 : v;
    v = k == 2 ? h.l2 : v;
    v = k == 3 ? 0x00450008u : v;                                   // 08 00 | 45 00
    v = k == 4 ? h.ver_len : v;
    v = k == 5 ? 0x06400040u : v;                                   // 40 00 | ttl 64, protocol 6
    v = k == 6 ? (ip_check | (h.saddr << 16)) : v;
    v = k == 7 ? ((h.saddr >> 16) | (h.daddr << 16)) : v;
    v = k == 8 ? ((h.daddr >> 16) | (h.ports << 16)) : v;
    v = k == 9 ? ((h.ports >> 16) | (h.seq_be << 16)) : v;
    v = k == 10 ? ((h.seq_be >> 16) | (h.ack_be << 16)) : v;
    v = k == 11 ? ((h.ack_be >> 16) | (h.off_flags << 16)) : v;
    v = k == 12 ? (h.win_be | (tcp_check << 16)) : v;
    v = k == 13 ? (h.o[0] << 16) : v;                               // urg 0
    v = k == 14 ? ((h.o[0] >> 16) | (h.o[1] << 16)) : v;
    v = k == 15 ? ((h.o[1] >> 16) | (h.o[2] << 16)) : v;
    v = k == 16 ? ((h.o[2] >> 16) | (h.o[3] << 16)) : v;
    v = k == 17 ? ((h.o[3] >> 16) | (h.o[4] << 16)) : v;
    v = k == 18 ? (h.o[4] >> 16) : v;
    return v;
}

// The payload bytes of chunk c of a segment on the destination's 16 B grid
// (zero outside the payload), and their word sum added to acc.
__device__ __forceinline__ v4u tx_chunk(const TxSeg &s, int c, uint32_t &acc) {
    const int js = 16 * c - s.a;                        // frame byte of the chunk's byte 0
    const uint64_t from = s.src + (int64_t)(js - s.H);  // its source address
    const uint64_t blk = from & ~15ull;
    const uint32_t sh = (uint32_t)from & 15u;           // the same for every chunk of the segment
    const uint64_t end = s.src + s.plen;
    v4u lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
    if ((int64_t)(blk + 16 - s.src) > 0 && (int64_t)(end - blk) > 0) lo = gload_nt(blk);
    if (sh && (int64_t)(blk + 32 - s.src) > 0 && (int64_t)(end - blk - 16) > 0) hi = gload_nt(blk + 16);
    const uint32_t ds = sh >> 2;
    const uint32_t x0 = ds == 0 ? lo.x : ds == 1 ? lo.y : ds == 2 ? lo.z : lo.w;
    const uint32_t x1 = ds == 0 ? lo.y : ds == 1 ? lo.z : ds == 2 ? lo.w : hi.x;
    const uint32_t x2 = ds == 0 ? lo.z : ds == 1 ? lo.w : ds == 2 ? hi.x : hi.y;
    const uint32_t x3 = ds == 0 ? lo.w : ds == 1 ? hi.x : ds == 2 ? hi.y : hi.z;
    const uint32_t x4 = ds == 0 ? hi.x : ds == 1 ? hi.y : ds == 2 ? hi.z : hi.w;
    const uint32_t bs = sh & 3u;
    v4u v;
    v.x = __builtin_amdgcn_alignbyte(x1, x0, bs);
    v.y = __builtin_amdgcn_alignbyte(x2, x1, bs);
    v.z = __builtin_amdgcn_alignbyte(x3, x2, bs);
    v.w = __builtin_amdgcn_alignbyte(x4, x3, bs);
    if (js < s.H || js + 16 > s.L) {                    // a chunk at an end of the payload
        v.x &= byte_mask(js, s.H, s.L);
        v.y &= byte_mask(js + 4, s.H, s.L);
        v.z &= byte_mask(js + 8, s.H, s.L);
        v.w &= byte_mask(js + 12, s.H, s.L);
    }
    acc = halves4(v, acc);
    return v;
}

// Stores chunk c: the frame's bytes only.
__device__ __forceinline__ void tx_store(const TxSeg &s, int c, const v4u &v) {
    const int js = 16 * c - s.a;
    const uint64_t at = (s.dst & ~15ull) + 16ull * (uint32_t)c;
    if (js >= 0 && js + 16 <= s.L) {
        *reinterpret_cast<gsv4u *>(at) = v;
        return;
    }
    store_part(at, v.x, -js, s.L - js);
    store_part(at + 4, v.y, -js - 4, s.L - js - 4);
    store_part(at + 8, v.z, -js - 8, s.L - js - 8);
    store_part(at + 12, v.w, -js - 12, s.L - js - 12);
}

constexpr int kTxHdrChunks = 6;     // (14 + 74 + 15) / 16: chunks that can hold header bytes

// G lanes per segment; 256-thread workgroups, 256 / G segments per trip.
template <int G>
__global__ __launch_bounds__(kBlock) void txbuild_kernel(const TxBuildParams p) {
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "8 lanes, a DPP row, half a wave or a wave per segment");
    constexpr int kPerWave = kWave / G;
    const int lane = threadIdx.x & (kWave - 1);
    const int t = lane & (G - 1);
    const int gbase = lane & ~(G - 1);                  // the group's first lane
    const uint32_t wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const uint32_t nwaves = gridDim.x * kWavesPerBlock;
    // the trip count is the wave's: every lane reaches every shuffle
    for (uint32_t first = wave * kPerWave; first < p.n; first += nwaves * kPerWave) {
        uint32_t i = first + (uint32_t)(lane / G);
        if (G == 64) i = __builtin_amdgcn_readfirstlane(i);
        const bool live = i < p.n;
        if (!live) i = first;

        // ---- the record, the descriptor, the link entry ----
        const uint64_t rec = (uint64_t)p.seg + 48ull * i;
        const v2u r0 = gload64(rec), r1 = gload64(rec + 8), r2 = gload64(rec + 16), r3 = gload64(rec + 24),
                    r4 = gload64(rec + 32), r5 = gload64(rec + 40);
        const v2u d = gload64((uint64_t)p.desc + 8ull * i);
        const uint64_t payload_off = ((uint64_t)r0.y << 32) | r0.x;
        const uint32_t plen = r5.x & 0xFFFFu, mss = r5.x >> 16;
        const uint32_t flags = r5.y & 0xFFu, form = (r5.y >> 8) & 0xFFu, wscale = (r5.y >> 16) & 0xFFu;
        const uint32_t link = r5.y >> 24;
        const bool syn = flags & 0x02u, ackf = flags & 0x10u;
        const uint32_t optlen = syn ? 20u : 12u;                             // tcp_out.c:21-60
        const uint32_t L = 54u + optlen + plen;
        const uint64_t off = (uint64_t)d.x << p.off_shift;

        uint32_t status = MTCP_GPU_TXB_BUILT;
        if (payload_off > p.payload_bytes || plen > p.payload_bytes - payload_off) status = MTCP_GPU_TXB_BAD_PAYLOAD;
        if ((d.y & 0xFFFFu) != L || (off & 1) || off > p.buf_len || L > p.buf_len - off)
            status = MTCP_GPU_TXB_BAD_DESC;
        if ((flags & ~0x1Fu) || form > 1 || link >= p.n_links || plen > p.max_mss + optlen || L > 65535u)
            status = MTCP_GPU_TXB_BAD_SEG;
        const bool ok = live && status == MTCP_GPU_TXB_BUILT;
        if (live && t == 0) *reinterpret_cast<gsu8 *>((uint64_t)p.status + i) = (uint8_t)status;

        TxSeg s;
        s.status = status;
        s.dst = (uint64_t)p.buf + off;
        s.src = (uint64_t)p.payload + payload_off;
        s.a = (int)(s.dst & 15);
        s.H = 54 + (int)optlen;
        s.L = (int)L;
        s.plen = plen;
        const int nch = ok ? (s.a + s.L + 15) >> 4 : 0;

        // ---- the payload: pass 0 holds the header chunks, the rest stream ----
        uint32_t acc = 0;
        v4u held = {0, 0, 0, 0};
        const bool hdr_lane = t < kTxHdrChunks && 16 * t - s.a < s.H;
        if (t < nch) {
            held = tx_chunk(s, t, acc);
            if (!hdr_lane) tx_store(s, t, held);
        }
#pragma unroll 2
        for (int c = t + G; c < nch; c += G) {
            const v4u v = tx_chunk(s, c, acc);
            tx_store(s, c, v);
        }

        // ---- the headers (every lane of the wave is here) ----
        const uint32_t lidx = link < p.n_links ? link : 0u;
        const uint64_t lk = (uint64_t)p.links + 12ull * lidx;
        TxHdr h;
        h.l0 = gload32(lk);
        h.l1 = gload32(lk + 4);
        h.l2 = gload32(lk + 8);
        h.saddr = r1.x;
        h.daddr = r1.y;
        h.ports = r2.x;
        h.seq_be = bswap32(r2.y);
        h.ack_be = ackf ? bswap32(r3.x) : 0u;                                // tcp_out.c:175-178
        const uint32_t ts_val = bswap32(r3.y), ts_ecr = bswap32(r4.x);
        const uint32_t tot_len = 40u + optlen + plen;
        h.ver_len = bswap16(tot_len) | (bswap16(r4.y >> 16) << 16);
        h.off_flags = (((20u + optlen) >> 2) << 4) | ((flags & 0x1Fu) << 8);
        h.win_be = bswap16(r4.y & 0xFFFFu);
        const uint32_t nop_ts = 0x0A080101u;                                 // 01 01 08 0a
        if (syn && form == 1) {                                              // tcp_out.c:79-114
            h.o[0] = 0x0402u | ((mss >> 8) << 16) | ((mss & 0xFFu) << 24);
            h.o[1] = nop_ts;
            h.o[2] = ts_val;
            h.o[3] = ts_ecr;
            h.o[4] = 0x00030301u | (wscale << 24);
        } else {                                                             // tcp_out.c:185-190, :118-122
            h.o[0] = nop_ts;
            h.o[1] = ts_val;
            h.o[2] = ts_ecr;
            h.o[3] = 0;                                                      // tcp_out.c:160: the memset's zeros
            h.o[4] = 0;
        }
        // ip_fast_csum over the 20 B header, check field zero (ip_out.c:94, :164)
        uint32_t s_ip = 0x0045u + 0x0040u + 0x0640u;
        s_ip = halves(h.ver_len, s_ip);
        s_ip = halves(h.saddr, s_ip);
        s_ip = halves(h.daddr, s_ip);
        const uint32_t ip_check = p.no_csum ? 0u : fold_csum(s_ip);

        // lane k < W of the group forms dwords k, W + k, ...; the TCP header
        // (frame bytes 34 .. H) and the pseudo header join the sum
        constexpr int W = G < 16 ? G : 16;               // lanes that hold header dwords
        constexpr int NH = (19 + W - 1) / W;             // dwords per such lane
        const int k0 = t & (W - 1);
        uint32_t hh[NH];
#pragma unroll
        for (int j = 0; j < NH; ++j) {
            hh[j] = tx_hdr_dword(h, j * W + k0, ip_check, 0);
            if (t < W) acc = halves(hh[j] & byte_mask(4 * (j * W + k0), 34, s.H), acc);
        }
        if (t == 0) {                                                        // tcp_util.c:157-190
            acc = halves(h.saddr, acc);
            acc = halves(h.daddr, acc);
            acc += 0x0600u + bswap16(20u + optlen + plen);
        }
        uint32_t tot;
        if (G == 8) {       // three row_shr steps: lanes 7 and 15 of a row hold their group's sum
            tot = acc;
            tot += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)tot, 0x111, 0xF, 0xF, true);
            tot += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)tot, 0x112, 0xF, 0xF, true);
            tot += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)tot, 0x114, 0xF, 0xF, true);
            tot = shfl32(tot, gbase + 7);
        } else {
            tot = row_sum(acc);
            if (G == 64)
                tot = shfl32(tot, 15) + shfl32(tot, 31) + shfl32(tot, 47) + shfl32(tot, 63);
            else if (G == 32)
                tot = shfl32(tot, gbase + 15) + shfl32(tot, gbase + 31);
            else
                tot = shfl32(tot, gbase + 15);
        }
        const uint32_t tcp_check = p.no_csum ? 0u : fold_csum(tot);
        if (k0 == 12 % W) hh[12 / W] |= tcp_check << 16;

        // header lane t takes frame dwords q .. q + 4 (q = (16 t - a) / 4,
        // rounded down) and shifts them onto the destination's grid
        const int js = 16 * t - s.a;
        const int q = js >> 2;                           // -4 .. 19
        uint32_t w[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int k = q + j;
            uint32_t v = 0;
#pragma unroll
            for (int m = 0; m < NH; ++m) {
                const uint32_t a = shfl32(hh[m], gbase + (k & (W - 1)));
                v = (k >= m * W && k < (m + 1) * W) ? a : v;
            }
            w[j] = k > 18 ? 0u : v;
        }
        if (ok && hdr_lane) {
            const uint32_t bs = (uint32_t)js & 3u;       // 0 or 2
            v4u v;
            v.x = __builtin_amdgcn_alignbyte(w[1], w[0], bs);
            v.y = __builtin_amdgcn_alignbyte(w[2], w[1], bs);
            v.z = __builtin_amdgcn_alignbyte(w[3], w[2], bs);
            v.w = __builtin_amdgcn_alignbyte(w[4], w[3], bs);
            // header dwords are zero from byte H on, held is zero before it
            v.x = (v.x & byte_mask(js, 0, s.H)) | held.x;
            v.y = (v.y & byte_mask(js + 4, 0, s.H)) | held.y;
            v.z = (v.z & byte_mask(js + 8, 0, s.H)) | held.z;
            v.w = (v.w & byte_mask(js + 12, 0, s.H)) | held.w;
            tx_store(s, t, v);
        }
    }
}

}  // namespace mg
