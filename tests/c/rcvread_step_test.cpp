// rcvread_step_test.cpp — mtcp_amd/csrc/rcvread_step.hpp on the CPU, a
// stand-alone program for g++ -fsanitize=address,undefined
// -fno-sanitize-recover=undefined (tests/test_rcvread_step_rules.py builds and
// runs it; nothing sanitized is loaded into Python).
//
//   fixture  every read and peek of tests/golden/rcvread_cases.bin
//            (tests/c/ref_rcvread_gen.c has the layout) as a batch of one
//            request: the records are built from the snapshot in front of the
//            event, the run in an arena of exact size holds the bytes the
//            reference returned; the result record, the records after and the
//            destination (a heap block of exact size) against the event's
//            values and the snapshot behind it;
//   random   batches over records of random bytes (every second one with the
//            fields of the BAD tests made sane) against a second, literal
//            restatement of the header's contract on the structs' fields:
//            every byte of the four record arrays, the results, the totals
//            and the destination.
//
// Prints one JSON line: per section the cases, the bad ones and the first bad
// line of this file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "rcvread_step_host.hpp"

namespace {

struct Section {
    const char *name;
    long cases = 0, bad = 0;
    int first_line = 0;
};
#define CHECK(sec, cond)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (!(sec).bad++) (sec).first_line = __LINE__; \
        }                                                  \
    } while (0)

uint64_t rng_s = 0x2545F4914F6CDD1Dull;
uint32_t rnd() {
    rng_s ^= rng_s << 13, rng_s ^= rng_s >> 7, rng_s ^= rng_s << 17;
    return (uint32_t)(rng_s >> 16);
}
uint32_t below(uint32_t n) { return rnd() % n; }

struct Reader {
    const std::vector<uint8_t> &raw;
    size_t pos = 0;
    uint32_t u32() {
        if (pos + 4 > raw.size()) abort();
        uint32_t v;
        memcpy(&v, &raw[pos], 4);
        pos += 4;
        return v;
    }
};

struct Snap {
    uint32_t head = 0, tail = 0, last = 0, head_seq = 0, merged = 0, rcv_wnd = 0, nfrag = 0;
    uint32_t frag[2 * 16] = {};
    void read(Reader &r) {
        head = r.u32(), tail = r.u32(), last = r.u32(), head_seq = r.u32(), merged = r.u32(), rcv_wnd = r.u32();
        nfrag = r.u32();
        if (nfrag > 16) abort();
        for (uint32_t k = 0; k < 2 * nfrag; ++k) frag[k] = r.u32();
    }
};

void fixture(const char *path, Section &sec) {
    FILE *f = fopen(path, "rb");
    if (!f) abort();
    std::vector<uint8_t> raw;
    uint8_t chunk[65536];
    for (size_t k; (k = fread(chunk, 1, sizeof(chunk), f)) > 0;) raw.insert(raw.end(), chunk, chunk + k);
    fclose(f);
    Reader r{raw};
    if (r.u32() != 0x52564352u || r.u32() != 1) abort();
    const uint32_t cases = r.u32();
    for (uint32_t c = 0; c < cases; ++c) {
        r.u32();
        const uint32_t size = r.u32(), init_seq = r.u32(), eff_mss = r.u32(), events = r.u32();
        Snap before;
        before.head_seq = init_seq, before.rcv_wnd = size;
        for (uint32_t e = 0; e < events; ++e) {
            const uint32_t kind = r.u32();
            if (kind == 0) {
                r.u32(), r.u32(), r.u32();
                before.read(r);
                continue;
            }
            const uint32_t len = r.u32(), nwa = r.u32(), ackq = r.u32();
            const int32_t ret = (int32_t)r.u32();
            const uint32_t nwa_after = r.u32(), ackq_after = r.u32(), freed = r.u32();
            const uint8_t *bytes = &raw[r.pos];
            if (ret > 0) r.pos += ((size_t)ret + 3) & ~(size_t)3;
            Snap after;
            after.read(r);
            const Snap b = before;
            before = after;
            if (b.nfrag > MTCP_GPU_RCV_MAX_FRAGS) continue;
            sec.cases++;
            // the records in front of the event
            mtcp_gpu_rcv_state st{};
            st.rcv_nxt = b.head_seq + b.merged, st.rcv_wnd = b.rcv_wnd, st.head_seq = b.head_seq, st.merged_len = b.merged;
            st.size = size, st.tcp_state = MTCP_GPU_RCV_ST_ESTABLISHED, st.nfrag = (uint8_t)b.nfrag;
            for (uint32_t k = 0; k < b.nfrag; ++k) st.frag[k].seq = b.frag[2 * k], st.frag[k].len = b.frag[2 * k + 1];
            mtcp_gpu_rcv_buf rb{};
            rb.data_off = 16, rb.size = size, rb.head_offset = b.head, rb.tail_offset = b.tail, rb.last_len = b.last;
            mtcp_gpu_ackgen_state tx{};
            tx.need_wnd_adv = (uint8_t)nwa;
            mtcp_gpu_ack_state snd{};
            snd.eff_mss = (uint16_t)eff_mss;
            std::vector<uint8_t> arena(16 + size + 16, 0xC3);
            if (ret > 0) memcpy(&arena[16 + b.head], bytes, (size_t)ret);
            const uint32_t room = std::min(len, size);
            std::vector<uint8_t> dst(7 + room, 0x5A);
            mtcp_gpu_rcvread_req rq{};
            rq.sid = 0, rq.len = len, rq.dst_off = 7;
            rq.flags = (kind == 2 ? MTCP_GPU_RCVREAD_PEEK : 0u) | (ackq ? MTCP_GPU_RCVREAD_ON_ACKQ : 0u);
            mtcp_gpu_rcvread_res res{};
            uint64_t total[2];
            rcvread_host::apply_batch(&rq, 1, 0, &st, &rb, &tx, &snd, arena.data(), arena.size(), dst.data(),
                                      dst.size(), &res, total);
            if (ret < 0) {
                CHECK(sec, res.verdict == MTCP_GPU_RCVREAD_EAGAIN && res.copylen == 0 && total[0] == 0 && total[1] == 0);
            } else {
                CHECK(sec, res.verdict == (kind == 2 ? MTCP_GPU_RCVREAD_PEEKED : MTCP_GPU_RCVREAD_READ));
                CHECK(sec, res.copylen == (uint32_t)ret && total[0] == 1 && total[1] == (uint64_t)ret);
                CHECK(sec, memcmp(&dst[7], bytes, (size_t)ret) == 0);
            }
            for (size_t k = 0; k < dst.size(); ++k)
                if (k < 7 || k >= 7 + (size_t)std::max(ret, 0)) CHECK(sec, dst[k] == 0x5A);
            CHECK(sec, rb.head_offset == after.head && rb.tail_offset == after.tail && rb.last_len == after.last);
            CHECK(sec, rb.data_off == 16 && rb.size == size && !rb.rsvd[0] && !rb.rsvd[1]);
            CHECK(sec, st.head_seq == after.head_seq && st.merged_len == after.merged && st.nfrag == after.nfrag);
            CHECK(sec, st.rcv_wnd == after.rcv_wnd && res.rcv_wnd == after.rcv_wnd && st.size == size);
            for (uint32_t k = 0; k < MTCP_GPU_RCV_MAX_FRAGS; ++k) {
                CHECK(sec, st.frag[k].seq == (k < after.nfrag ? after.frag[2 * k] : 0u));
                CHECK(sec, st.frag[k].len == (k < after.nfrag ? after.frag[2 * k + 1] : 0u));
            }
            CHECK(sec, tx.need_wnd_adv == nwa_after);
            const uint32_t flags = (after.merged ? MTCP_GPU_RCVREAD_MORE : 0u) |
                                   (ackq_after && !ackq ? MTCP_GPU_RCVREAD_WND_ADV : 0u) |
                                   (freed ? MTCP_GPU_RCVREAD_FRAG_FREED : 0u);
            CHECK(sec, res.flags == flags && res.sid == 0 && res.rsvd == 0);
        }
    }
    if (r.pos != raw.size()) abort();
}

// The header's contract once more, on the structs' fields, for one request
// that won its claim or lost it (dup).
void restated(const mtcp_gpu_rcvread_req &q, bool dup, uint32_t max_id, mtcp_gpu_rcv_state *state,
              mtcp_gpu_rcv_buf *rbuf, mtcp_gpu_ackgen_state *tx, const mtcp_gpu_ack_state *snd,
              const std::vector<uint8_t> &arena, std::vector<uint8_t> &dst, mtcp_gpu_rcvread_res &r, uint64_t total[2]) {
    memset(&r, 0, sizeof(r));
    r.sid = q.sid;
    r.verdict = MTCP_GPU_RCVREAD_BAD_REQ;
    if (q.sid > max_id || q.rsvd[0] || q.rsvd[1] || q.rsvd[2] || (q.flags & ~3u)) return;
    mtcp_gpu_rcv_state &s = state[q.sid];
    mtcp_gpu_rcv_buf &b = rbuf[q.sid];
    if (q.dst_off > dst.size() || std::min(q.len, b.size) > dst.size() - q.dst_off) return;
    r.verdict = MTCP_GPU_RCVREAD_DUP;
    if (dup) return;
    r.verdict = MTCP_GPU_RCVREAD_BAD_STATE;
    if (s.rsvd || s.nfrag > 4 || s.size > (1u << 30) || s.merged_len > s.size) return;
    for (uint32_t k = 0; k < s.nfrag; ++k)
        if (s.frag[k].len >= (1u << 31)) return;
    if (b.rsvd[0] || b.rsvd[1] || b.size == 0 || b.size > (1u << 30) || b.data_off > arena.size() ||
        b.size > arena.size() - b.data_off || b.head_offset > b.tail_offset || b.tail_offset > b.size ||
        b.last_len != b.tail_offset - b.head_offset)
        return;
    const uint32_t copylen = std::min(s.merged_len, q.len);
    if (s.size != b.size || s.merged_len > b.last_len) return;
    if (s.merged_len > 0 && (s.nfrag == 0 || s.frag[0].seq != s.head_seq)) return;
    if (copylen > s.frag[0].len) return;
    r.rcv_wnd = s.rcv_wnd, r.flags = s.merged_len ? MTCP_GPU_RCVREAD_MORE : 0;
    r.verdict = MTCP_GPU_RCVREAD_DEFER_STATE;
    if (s.tcp_state != 4) return;
    r.verdict = MTCP_GPU_RCVREAD_EAGAIN;
    if (copylen == 0) return;
    memcpy(&dst[q.dst_off], &arena[b.data_off + b.head_offset], copylen);
    total[0]++, total[1] += copylen;
    r.copylen = copylen;
    r.verdict = MTCP_GPU_RCVREAD_PEEKED;
    if (q.flags & MTCP_GPU_RCVREAD_PEEK) return;
    r.verdict = MTCP_GPU_RCVREAD_READ, r.flags = 0;
    b.head_offset += copylen, b.last_len -= copylen;
    s.head_seq += copylen, s.merged_len -= copylen;
    if (copylen == s.frag[0].len) {
        for (uint32_t k = 0; k + 1 < s.nfrag; ++k) s.frag[k] = s.frag[k + 1];
        s.nfrag--;
        s.frag[s.nfrag].seq = s.frag[s.nfrag].len = 0;
        r.flags |= MTCP_GPU_RCVREAD_FRAG_FREED;
    } else {
        s.frag[0].seq += copylen, s.frag[0].len -= copylen;
    }
    s.rcv_wnd = s.size - s.merged_len;
    r.rcv_wnd = s.rcv_wnd;
    if (tx && tx[q.sid].need_wnd_adv == 1 && s.rcv_wnd > snd[q.sid].eff_mss && !(q.flags & MTCP_GPU_RCVREAD_ON_ACKQ))
        tx[q.sid].need_wnd_adv = 0, r.flags |= MTCP_GPU_RCVREAD_WND_ADV;
    if (s.merged_len) r.flags |= MTCP_GPU_RCVREAD_MORE;
}

template <class T>
void fill_random(std::vector<T> &v) {
    uint8_t *p = reinterpret_cast<uint8_t *>(v.data());
    for (size_t k = 0; k < v.size() * sizeof(T); ++k) p[k] = (uint8_t)rnd();
}

void random_batches(long rounds, Section &sec) {
    constexpr uint32_t kStreams = 12, kReq = 16, kArena = 2048, kDst = 16384;
    for (long it = 0; it < rounds; ++it) {
        std::vector<mtcp_gpu_rcv_state> state(kStreams);
        std::vector<mtcp_gpu_rcv_buf> rbuf(kStreams);
        std::vector<mtcp_gpu_ackgen_state> tx(kStreams);
        std::vector<mtcp_gpu_ack_state> snd(kStreams);
        std::vector<uint8_t> arena(kArena), dst(kDst, 0x5A);
        std::vector<mtcp_gpu_rcvread_req> req(kReq);
        fill_random(state), fill_random(rbuf), fill_random(tx), fill_random(snd), fill_random(arena), fill_random(req);
        for (uint32_t i = 0; i < kStreams; i += 2) {
            const uint32_t size = 1 + below(512), head = below(size), last = below(size - head + 1);
            const uint32_t merged = below(last + 1);
            rbuf[i] = mtcp_gpu_rcv_buf{below(kArena - size), size, head, head + last, last, {0, 0}};
            mtcp_gpu_rcv_state &s = state[i];
            s.rsvd = 0, s.size = size, s.merged_len = merged, s.nfrag = (uint8_t)(1 + below(4));
            for (auto &fr : s.frag) fr.len &= 0x7FFFFFFFu;
            s.tcp_state = below(4) ? 4 : (uint8_t)below(11);
            if (below(8)) s.frag[0].seq = s.head_seq, s.frag[0].len = merged + (below(2) ? below(3) : 0);
            tx[i].need_wnd_adv = (uint8_t)below(3), snd[i].eff_mss = (uint16_t)below(size);
        }
        // accepted ranges apart: request i owns [1024 i, 1024 (i + 1))
        for (uint32_t i = 0; i < kReq; ++i)
            if (below(8)) {
                req[i].rsvd[0] = req[i].rsvd[1] = req[i].rsvd[2] = 0;
                req[i].flags &= 3, req[i].sid = below(kStreams + 1), req[i].len = below(500);
                req[i].dst_off = 1024ull * i + below(500);
            } else if (below(2)) {
                req[i].dst_off = kDst - below(40);     // at the region's end: the bound's test
                req[i].rsvd[0] = req[i].rsvd[1] = req[i].rsvd[2] = 0, req[i].flags &= 3, req[i].sid = below(kStreams);
                req[i].len = below(64);
            }
        const bool has_tx = below(4) != 0;
        auto state2 = state;
        auto rbuf2 = rbuf;
        auto tx2 = tx;
        auto dst2 = dst;
        std::vector<mtcp_gpu_rcvread_res> res(kReq), res2(kReq);
        uint64_t total[2], total2[2] = {0, 0};
        const uint32_t max_id = kStreams - 1;
        rcvread_host::apply_batch(req.data(), kReq, max_id, state.data(), rbuf.data(), has_tx ? tx.data() : nullptr,
                                  has_tx ? snd.data() : nullptr, arena.data(), arena.size(), dst.data(), dst.size(),
                                  res.data(), total);
        for (uint32_t i = 0; i < kReq; ++i) {
            bool dup = false;
            for (uint32_t j = 0; j < i; ++j) dup |= req[j].sid == req[i].sid;
            restated(req[i], dup, max_id, state2.data(), rbuf2.data(), has_tx ? tx2.data() : nullptr, snd.data(), arena,
                     dst2, res2[i], total2);
        }
        sec.cases++;
        CHECK(sec, memcmp(res.data(), res2.data(), 16 * kReq) == 0);
        CHECK(sec, memcmp(state.data(), state2.data(), 64 * kStreams) == 0);
        CHECK(sec, memcmp(rbuf.data(), rbuf2.data(), 32 * kStreams) == 0);
        CHECK(sec, memcmp(tx.data(), tx2.data(), 32 * kStreams) == 0);
        CHECK(sec, dst == dst2 && total[0] == total2[0] && total[1] == total2[1]);
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s tests/golden/rcvread_cases.bin\n", argv[0]);
        return 2;
    }
    Section fx{"fixture"}, rn{"random"};
    fixture(argv[1], fx);
    random_batches(100000, rn);
    printf("{\"fixture\": {\"cases\": %ld, \"bad\": %ld, \"first_line\": %d}, "
           "\"random\": {\"cases\": %ld, \"bad\": %ld, \"first_line\": %d}}\n",
           fx.cases, fx.bad, fx.first_line, rn.cases, rn.bad, rn.first_line);
    return 0;
}
