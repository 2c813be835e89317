// sndwrite_step_test.cpp — TEST INFRASTRUCTURE ONLY: the write's step text
// (mtcp_amd/csrc/sndwrite_step.hpp through sndwrite_step_host.hpp) against a
// second, literal restatement of include/mtcp_gpu_sndwrite.h on the struct
// fields.  A stand-alone program: tests/test_sndwrite_step_rules.py builds it
// with g++ -fsanitize=address,undefined and runs it directly.
//
//   1. the fixture (argv[1], tests/golden/sndwrite_cases.bin): every SBPut as a
//      batch of one request on a heap chunk of exact size, every SBRemove as the
//      record update the ACK walk makes; the return value, head_off, tail_off,
//      len, head_seq and every byte of the chunk after every operation;
//   2. random batches of random record bytes (100 000), snd_wnd at 0, 1,
//      2^31 - 1, 2^31 and 2^32 - 1 and len at 0, 1 and 2^31 - 1 among them.
//
// Prints one JSON line; "bad" counts mismatches, "first_line" is the source line
// of the first one.
#include <stdio.h>
#include <stdlib.h>

#include "sndwrite_step_host.hpp"

namespace {

uint64_t rng_s = 0x2545F4914F6CDD1Dull;
uint32_t rnd() {
    rng_s ^= rng_s << 13, rng_s ^= rng_s >> 7, rng_s ^= rng_s << 17;
    return (uint32_t)(rng_s >> 16);
}
uint32_t below(uint32_t n) { return rnd() % n; }

struct Tally {
    uint64_t cases = 0, bad = 0;
    int first_line = 0;
    void fail(int line) {
        if (!bad++) first_line = line;
    }
};
#define EXPECT(t, c)              \
    do {                          \
        if (!(c)) (t).fail(__LINE__); \
    } while (0)

// ---- the second restatement: the header's rules on the struct fields ------------------------------
struct Ref {
    mtcp_gpu_sndwrite_res res;
    uint32_t seg_sid;
    bool moved, copied;
    uint64_t move_to, move_from, move_len, dst, src, len;
};

Ref ref_one(const mtcp_gpu_sndwrite_req &q, bool dup, uint32_t max_id, mtcp_gpu_ack_state *snd,
            mtcp_gpu_datagen_state *dtx, uint64_t src_bytes, uint64_t payload_bytes) {
    Ref r{};
    r.res.sid = q.sid, r.seg_sid = MTCP_GPU_FLOW_NONE;
    auto verdict = [&](int v) {
        r.res.verdict = (uint8_t)v;
        return r;
    };
    if (q.sid > max_id || q.flags || q.rsvd[0] || q.rsvd[1] || q.rsvd[2] || q.len > 0x7FFFFFFFu ||
        (unsigned __int128)q.src_off + q.len > src_bytes)
        return verdict(MTCP_GPU_SNDWRITE_BAD_REQ);
    if (dup) return verdict(MTCP_GPU_SNDWRITE_DUP);
    mtcp_gpu_ack_state &s = snd[q.sid];
    mtcp_gpu_datagen_state &d = dtx[q.sid];
    const uint32_t head_off = s.sb_len == 0 ? 0u : s.sb_head_seq - d.sb_base_seq;
    bool bad = s.rsvd != 0 || s.eff_mss == 0 || s.wscale_peer > 31 || s.sb_size > (1u << 30) || s.sb_len > s.sb_size;
    bad = bad || d.rsvd[0] || d.rsvd[1] || d.on_send_list > 1 || d.on_control_list > 1;
    if (!bad && s.has_sndbuf)
        bad = s.sb_size == 0 || (unsigned __int128)d.sb_off + s.sb_size > payload_bytes ||
              head_off > s.sb_size - s.sb_len;
    if (bad) return verdict(MTCP_GPU_SNDWRITE_BAD_STATE);
    auto with_wnd = [&](int v) {
        r.res.snd_wnd = s.snd_wnd;
        if (s.snd_wnd > 0) r.res.flags |= MTCP_GPU_SNDWRITE_ROOM;
        return verdict(v);
    };
    if (s.tcp_state != 4) return with_wnd(MTCP_GPU_SNDWRITE_DEFER_STATE);
    if (q.len == 0) return with_wnd(MTCP_GPU_SNDWRITE_ZERO);
    const int64_t wnd = (int64_t)(int32_t)s.snd_wnd, len = (int64_t)(int32_t)q.len;
    const int64_t sndlen = wnd < len ? wnd : len;
    if (sndlen <= 0) return with_wnd(MTCP_GPU_SNDWRITE_EAGAIN);
    if (!s.has_sndbuf) return with_wnd(MTCP_GPU_SNDWRITE_NO_SNDBUF);
    const int64_t space = (int64_t)s.sb_size - s.sb_len;
    const int64_t to_put = sndlen < space ? sndlen : space;
    if (to_put == 0) {
        s.snd_wnd = (uint32_t)space;
        return with_wnd(MTCP_GPU_SNDWRITE_FULL);
    }
    const uint64_t tail_off = (uint64_t)head_off + s.sb_len;
    r.copied = true, r.src = q.src_off, r.len = (uint64_t)to_put;
    if (tail_off + (uint64_t)to_put < s.sb_size) {
        r.dst = d.sb_off + tail_off;
        if (s.sb_len == 0) d.sb_base_seq = s.sb_head_seq;
    } else {
        r.moved = head_off != 0 && s.sb_len != 0;
        r.move_to = d.sb_off, r.move_from = d.sb_off + head_off, r.move_len = s.sb_len;
        r.dst = d.sb_off + s.sb_len;
        d.sb_base_seq = s.sb_head_seq;
        r.res.flags |= MTCP_GPU_SNDWRITE_COMPACTED;
    }
    s.sb_len += (uint32_t)to_put;
    s.snd_wnd = s.sb_size - s.sb_len;
    if (!d.on_send_list) r.res.flags |= MTCP_GPU_SNDWRITE_SEND_LIST_ADD;
    d.on_send_list = 1;
    r.res.written = (uint32_t)to_put, r.seg_sid = q.sid;
    return with_wnd(MTCP_GPU_SNDWRITE_WRITTEN);
}

void ref_batch(const mtcp_gpu_sndwrite_req *req, uint32_t n, uint32_t max_id, mtcp_gpu_ack_state *snd,
               mtcp_gpu_datagen_state *dtx, const uint8_t *src, uint64_t src_bytes, uint8_t *payload,
               uint64_t payload_bytes, mtcp_gpu_sndwrite_res *wres, uint32_t *seg_sid, uint64_t total[2]) {
    std::vector<Ref> refs(n);
    total[0] = total[1] = 0;
    for (uint32_t i = 0; i < n; ++i) {
        bool dup = false;
        for (uint32_t j = 0; j < i; ++j) dup |= req[j].sid == req[i].sid;
        refs[i] = ref_one(req[i], dup, max_id, snd, dtx, src_bytes, payload_bytes);
        wres[i] = refs[i].res, seg_sid[i] = refs[i].seg_sid;
        if (refs[i].copied) total[0]++, total[1] += refs[i].len;
    }
    for (const Ref &r : refs)
        if (r.moved) memmove(payload + r.move_to, payload + r.move_from, r.move_len);
    for (const Ref &r : refs)
        if (r.copied) memcpy(payload + r.dst, src + r.src, r.len);
}

// ---- 1. the fixture ---------------------------------------------------------------------------------
std::vector<uint8_t> file;
size_t pos;
uint32_t u32() {
    uint32_t v = 0;
    if (pos + 4 <= file.size()) memcpy(&v, &file[pos], 4);
    pos += 4;
    return v;
}

void run_fixture(Tally &t) {
    pos = 0;
    const uint32_t magic = u32(), version = u32(), ncases = u32();
    EXPECT(t, magic == 0x57444E53u && version == 1);
    for (uint32_t c = 0; c < ncases; ++c) {
        const uint32_t family = u32(), size = u32(), init_seq = u32(), nops = u32();
        (void)family;
        // the chunk as a heap block of exact size, 16 B aligned as the arena is
        uint8_t *chunk = static_cast<uint8_t *>(aligned_alloc(16, (size + 15) & ~15u));
        memset(chunk, 0xEE, size);
        mtcp_gpu_ack_state snd{};
        mtcp_gpu_datagen_state dtx{};
        snd.sb_head_seq = init_seq, snd.sb_size = size, snd.eff_mss = 1448, snd.tcp_state = 4, snd.has_sndbuf = 1;
        dtx.sb_base_seq = init_seq ^ 0x55u;                          // stale: the buffer is empty
        uint32_t serial = 0, prev_tail = 0;                          // tail_off as the operation before left it
        for (uint32_t k = 0; k < nops; ++k) {
            const uint32_t kind = u32(), len = u32();
            const int32_t ret = (int32_t)u32();
            const uint32_t head_off = u32(), tail_off = u32(), blen = u32();
            u32(), u32();                                            // cum_len: not mirrored
            const uint32_t head_seq = u32();
            if (kind == 0) {
                std::vector<uint8_t> src((len + 15) & ~15u);
                for (uint32_t i = 0; i < len; ++i) src[i] = (uint8_t)(c * 113 + serial * 29 + i * 5 + (i >> 8));
                serial++;
                mtcp_gpu_sndwrite_req q{};
                q.len = len;
                mtcp_gpu_sndwrite_res res{};
                uint32_t seg_sid = 7, seg_start[2] = {7, 7}, seg_stop = 7, nseg = 7;
                uint64_t total[2];
                const uint32_t on_before = dtx.on_send_list;
                snd.snd_wnd = size;                                  // an open window: SBPut's own clamp decides
                sndwrite_host::apply_batch(&q, 1, 0, &snd, &dtx, src.data(), src.size(), chunk, size, &res, &seg_sid,
                                           seg_start, &seg_stop, &nseg, total);
                if (ret > 0) {
                    EXPECT(t, res.verdict == MTCP_GPU_SNDWRITE_WRITTEN && res.written == (uint32_t)ret);
                    EXPECT(t, seg_sid == 0 && total[0] == 1 && total[1] == (uint64_t)ret && dtx.on_send_list == 1);
                    EXPECT(t, !(res.flags & MTCP_GPU_SNDWRITE_SEND_LIST_ADD) == (on_before != 0));
                    EXPECT(t, !(res.flags & MTCP_GPU_SNDWRITE_COMPACTED) == (prev_tail + (uint32_t)ret < size));   // :130
                } else {
                    EXPECT(t, ret == -2 && res.verdict == MTCP_GPU_SNDWRITE_FULL && res.written == 0);
                    EXPECT(t, seg_sid == MTCP_GPU_FLOW_NONE && total[0] == 0 && total[1] == 0);
                }
                EXPECT(t, res.snd_wnd == size - blen && snd.snd_wnd == size - blen);
                EXPECT(t, !(res.flags & MTCP_GPU_SNDWRITE_ROOM) == (size == blen));
                EXPECT(t, seg_start[0] == 0 && seg_start[1] == 0 && seg_stop == 0 && nseg == 1);
            } else if (ret > 0) {
                // SBRemove as the ACK walk mirrors it: head_seq and len; d_dtx keeps its bytes
                snd.sb_head_seq += (uint32_t)ret, snd.sb_len -= (uint32_t)ret;
            }
            const uint32_t got_head = snd.sb_len == 0 ? 0u : snd.sb_head_seq - dtx.sb_base_seq;
            EXPECT(t, snd.sb_len == blen && snd.sb_head_seq == head_seq);
            // an empty buffer's tail_off is left where it was by a put (it is reset by the remove that empties it)
            EXPECT(t, got_head == head_off && (blen == 0 || got_head + snd.sb_len == tail_off));
            EXPECT(t, pos + size <= file.size() && memcmp(chunk, &file[pos], size) == 0);
            pos += size;
            prev_tail = tail_off;
            t.cases++;
        }
        free(chunk);
    }
    EXPECT(t, pos == file.size());
}

// ---- 2. random batches of random record bytes -------------------------------------------------------
void fill_random(void *p, size_t n) {
    uint8_t *b = static_cast<uint8_t *>(p);
    for (size_t i = 0; i < n; ++i) b[i] = (uint8_t)rnd();
}

void run_random(Tally &t, uint32_t batches) {
    constexpr uint32_t kStreams = 4, kSlot = 256, kSrc = 512, kReq = 6;
    static const uint32_t wnds[] = {0, 1, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu, 40, 300};
    static const uint32_t lens[] = {0, 1, 0x7FFFFFFFu, 15, 16, 17, 100, kSrc};
    for (uint32_t b = 0; b < batches; ++b) {
        mtcp_gpu_ack_state snd[2][kStreams];
        mtcp_gpu_datagen_state dtx[2][kStreams];
        mtcp_gpu_sndwrite_req req[kReq];
        fill_random(snd[0], sizeof snd[0]), fill_random(dtx[0], sizeof dtx[0]), fill_random(req, sizeof req);
        for (uint32_t i = 0; i < kStreams; ++i) {
            mtcp_gpu_ack_state &s = snd[0][i];
            mtcp_gpu_datagen_state &d = dtx[0][i];
            if (below(6)) {
                s.rsvd = 0, s.wscale_peer = (uint8_t)below(32), s.eff_mss = (uint16_t)(1 + below(1500));
                s.tcp_state = below(6) ? 4 : (uint8_t)below(11), s.has_sndbuf = below(8) ? (uint8_t)(1 + below(2) * 6) : 0;
                d.rsvd[0] = d.rsvd[1] = 0, d.on_send_list = (uint8_t)below(2), d.on_control_list = (uint8_t)below(2);
                s.snd_wnd = wnds[below(7)];
            }
            // disjoint chunks: inside the stream's own slot, or outside any arena
            if (below(6)) {
                s.sb_size = below(kSlot - 15 + 1);
                s.sb_len = below(8) ? below(s.sb_size + 1) : s.sb_size + below(3);
                d.sb_off = (uint64_t)i * kSlot + below(16);
                if (below(6) && s.sb_size) d.sb_base_seq = s.sb_head_seq - below(s.sb_size - (s.sb_len < s.sb_size ? s.sb_len : s.sb_size) + 1);
            } else {
                d.sb_off |= 1ull << 63;
            }
        }
        for (uint32_t i = 0; i < kReq; ++i) {
            if (below(8)) req[i].sid = below(kStreams + 1);
            if (below(8)) req[i].flags = 0, req[i].rsvd[0] = req[i].rsvd[1] = req[i].rsvd[2] = 0;
            if (below(8)) {
                req[i].len = lens[below(8)];
                req[i].src_off = below(kSrc - (req[i].len < kSrc ? req[i].len : kSrc) + 2);
            }
        }
        memcpy(snd[1], snd[0], sizeof snd[0]), memcpy(dtx[1], dtx[0], sizeof dtx[0]);
        // heap blocks of exact size: a load or store past them ends the program
        uint8_t *src = static_cast<uint8_t *>(malloc(kSrc));
        uint8_t *pay[2] = {static_cast<uint8_t *>(malloc(kStreams * kSlot)), static_cast<uint8_t *>(malloc(kStreams * kSlot))};
        fill_random(src, kSrc), fill_random(pay[0], kStreams * kSlot), memcpy(pay[1], pay[0], kStreams * kSlot);
        mtcp_gpu_sndwrite_res wres[2][kReq];
        uint32_t seg_sid[2][kReq], seg_start[kReq + 1], seg_stop[kReq], nseg = 99;
        uint64_t total[2][2];
        sndwrite_host::apply_batch(req, kReq, kStreams - 1, snd[0], dtx[0], src, kSrc, pay[0], kStreams * kSlot, wres[0],
                                   seg_sid[0], seg_start, seg_stop, &nseg, total[0]);
        ref_batch(req, kReq, kStreams - 1, snd[1], dtx[1], src, kSrc, pay[1], kStreams * kSlot, wres[1], seg_sid[1],
                  total[1]);
        EXPECT(t, memcmp(wres[0], wres[1], sizeof wres[0]) == 0);
        EXPECT(t, memcmp(snd[0], snd[1], sizeof snd[0]) == 0 && memcmp(dtx[0], dtx[1], sizeof dtx[0]) == 0);
        EXPECT(t, memcmp(pay[0], pay[1], kStreams * kSlot) == 0);
        EXPECT(t, memcmp(seg_sid[0], seg_sid[1], sizeof seg_sid[0]) == 0 && nseg == kReq);
        EXPECT(t, total[0][0] == total[1][0] && total[0][1] == total[1][1]);
        for (uint32_t i = 0; i < kReq; ++i) EXPECT(t, seg_start[i] == 0 && seg_stop[i] == 0);
        EXPECT(t, seg_start[kReq] == 0);
        free(src), free(pay[0]), free(pay[1]);
        t.cases++;
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    file.resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    if (fread(file.data(), 1, file.size(), f) != file.size()) return 2;
    fclose(f);
    Tally fx, rn;
    run_fixture(fx);
    run_random(rn, 100000);
    printf("{\"fixture\": {\"cases\": %llu, \"bad\": %llu, \"first_line\": %d}, "
           "\"random\": {\"cases\": %llu, \"bad\": %llu, \"first_line\": %d}}\n",
           (unsigned long long)fx.cases, (unsigned long long)fx.bad, fx.first_line, (unsigned long long)rn.cases,
           (unsigned long long)rn.bad, rn.first_line);
    return fx.bad || rn.bad ? 1 : 0;
}
