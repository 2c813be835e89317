// ackgen_step_test.cpp — mtcp_amd/csrc/ackgen_step.hpp on the CPU, a stand-alone
// program for g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// (tests/test_ackgen_step_rules.py builds and runs it; nothing sanitized is
// loaded into Python).  host_stream below is the kernels' order of calls for
// one stream: the BAD test, the fold, the plan, the records, the commit.
//
//   fixture  every case of tests/golden/ackgen_cases.bin
//            (tests/c/ref_ackgen_gen.c has the layout): the options as
//            placement words (ACK_OPT_WACK as is_wack on entry), the case's
//            slot budget as the room; every field of every record against the
//            reference's frame bytes, the record after against the reference's
//            stream after, on_ack_list against the result;
//   random   tx records, states and placement words of random bytes (every
//            second record with the fields of the BAD test made sane): the fold
//            over the masks equals the fold packet by packet, a BAD stream
//            changes nothing, the fixed bytes never change, the emitted
//            records are a prefix of the planned ones, the room rule's closed
//            form equals the rule applied record by record (cut by seg_cap, by
//            buf_len and by the 32-bit offset), and the sanitizers stay silent
//            (no shift goes past the width).
//
// Prints one JSON line: per section the cases, the bad ones and the first bad
// line of this file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <array>
#include <vector>

#include "../../mtcp_amd/csrc/ackgen_step.hpp"

namespace {

struct Section {
    const char *name;
    long cases = 0, bad = 0;
    int first_line = 0;
};
#define CHECK(sec, cond)                              \
    do {                                              \
        if (!(cond)) {                                \
            if (!(sec).bad++) (sec).first_line = __LINE__; \
        }                                             \
    } while (0)

uint64_t rng_s = 0x2545F4914F6CDD1Dull;
uint32_t rnd() {
    rng_s ^= rng_s << 13, rng_s ^= rng_s >> 7, rng_s ^= rng_s << 17;
    return (uint32_t)(rng_s >> 16);
}
uint32_t rd32(const uint8_t *p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
uint16_t rd16(const uint8_t *p) {
    uint16_t v;
    memcpy(&v, p, 2);
    return v;
}
uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
uint32_t be16(const uint8_t *p) { return (uint32_t)p[0] << 8 | p[1]; }

struct Walk {   // d_state[id] and d_snd[id].snd_nxt
    uint32_t snd_nxt, rcv_nxt, rcv_wnd, head_seq, merged_len, ts_recent;
};
struct Out {
    std::vector<std::array<uint32_t, 12>> recs;
    uint32_t res[4];
};

uint32_t fold_serial(uint32_t f, const std::vector<uint32_t> &w) {
    for (uint32_t x : w) f = mg::ackgen_fold(f, x);
    return f;
}
uint32_t fold_masks(uint32_t f, const std::vector<uint32_t> &w) {
    for (size_t base = 0; base < w.size(); base += 64) {
        uint64_t now = 0, agg = 0, put = 0;
        for (size_t i = base; i < w.size() && i < base + 64; ++i) {
            const uint32_t fl = w[i] >> 24;
            if (fl & MTCP_GPU_RCV_ACK_NOW) now |= 1ull << (i - base);
            if (fl & MTCP_GPU_RCV_ACK_AGGREGATE) agg |= 1ull << (i - base);
            if (mg::ackgen_is_put(w[i])) put |= 1ull << (i - base);
        }
        f = mg::ackgen_fold_masks(f, now, agg, put);
    }
    return f;
}

// One stream as the kernels run it, its first record being S of a call with
// room for E.  tx: the record's 32 B, updated.
void host_stream(uint8_t tx[32], const std::vector<uint32_t> &w, bool masks, bool deferred, const Walk &k, uint32_t S,
                 uint32_t E, uint32_t cur_ts, uint32_t n_links, Out &o) {
    mg::AckGenTx t;
    memcpy(&t, tx, 32);
    o.recs.clear();
    mg::AckGenPlan pl;
    if (mg::ackgen_bad(t, n_links)) {
        pl = mg::ackgen_plan_none(MTCP_GPU_ACKGEN_BAD);
    } else {
        const uint32_t f0 = (t.id_cnt >> 16) & 63u;
        const uint32_t f = masks ? fold_masks(f0, w) : fold_serial(f0, w);
        pl = mg::ackgen_plan(t, f, deferred, k.rcv_nxt, k.rcv_wnd, k.head_seq, k.merged_len, k.ts_recent, k.snd_nxt);
    }
    const uint32_t planned = mg::ackgen_planned(pl);
    for (uint32_t i = 0; i < planned && S + i < E; ++i) {
        std::array<uint32_t, 12> r;
        mg::ackgen_record(pl, i, cur_ts, r.data());
        o.recs.push_back(r);
    }
    uint32_t t3[3];
    bool store_ts;
    mg::ackgen_commit(pl, S, E, S < E ? S : E, cur_ts, t3, &store_ts, o.res);
    if (mg::ackgen_status(pl) >= MTCP_GPU_ACKGEN_DEFERRED) {
        memcpy(tx + 12, &t3[0], 4), memcpy(tx + 16, &t3[1], 4);
        if (store_ts) memcpy(tx + 20, &t3[2], 4);
    }
}

void fixture(Section &sec, const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    std::vector<uint8_t> raw;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + got);
    fclose(f);
    if (raw.size() < 16 || rd32(&raw[0]) != 0x474B4341u || rd32(&raw[4]) != 1) exit(2);
    const uint32_t cases = rd32(&raw[8]);
    size_t at = 16;
    for (uint32_t c = 0; c < cases; ++c) {
        if (at + 68 > raw.size()) exit(2);
        uint8_t tx[32];
        memcpy(tx, &raw[at], 32);
        Walk k;
        memcpy(&k, &raw[at + 32], 24);
        const uint32_t cur_ts = rd32(&raw[at + 56]);
        const uint32_t budget = rd16(&raw[at + 60]), n_opts = rd16(&raw[at + 62]), n_frames = rd16(&raw[at + 64]);
        const uint32_t listed = raw[at + 67];
        at += 68;
        const size_t frames_at = at + ((n_opts + 3) & ~3u), after_at = frames_at + 66ull * n_frames;
        if (after_at + 56 > raw.size()) exit(2);
        std::vector<uint32_t> w;
        for (uint32_t i = 0; i < n_opts; ++i) {
            const uint8_t o = raw[at + i];
            if (o == 0) w.push_back(MTCP_GPU_RCV_ACK_NOW << 24 | MTCP_GPU_RCV_SEQ_AHEAD << 16);
            else if (o == 1) w.push_back(MTCP_GPU_RCV_ACK_AGGREGATE << 24 | MTCP_GPU_RCV_SEQ_OLD << 16);
            else tx[15] = 1;                                       // ACK_OPT_WACK: tcp_out.c:931-933
        }
        for (int masks = 0; masks < 2; ++masks) {
            uint8_t t2[32];
            memcpy(t2, tx, 32);
            Out o;
            host_stream(t2, w, masks != 0, false, k, 0, budget, cur_ts, 3, o);
            sec.cases++;
            CHECK(sec, o.recs.size() == n_frames);
            for (size_t i = 0; i < o.recs.size() && i < n_frames; ++i) {
                const uint8_t *fr = &raw[frames_at + 66 * i];
                const uint32_t *r = o.recs[i].data();
                CHECK(sec, r[0] == 0 && r[1] == 0 && r[10] == 0);
                CHECK(sec, r[2] == rd32(fr + 26) && r[3] == rd32(fr + 30) && r[4] == rd32(fr + 34));
                CHECK(sec, r[5] == be32(fr + 38) && r[6] == be32(fr + 42));
                CHECK(sec, r[7] == be32(fr + 58) && r[8] == be32(fr + 62));
                CHECK(sec, (r[9] & 0xFFFFu) == be16(fr + 48) && (r[9] >> 16) == be16(fr + 18));
                CHECK(sec, (r[11] & 0xFFu) == fr[47] && ((r[11] >> 8) & 0xFFu) == 1 && ((r[11] >> 16) & 0xFFu) == 0);
                CHECK(sec, (r[11] >> 24) == fr[5] && fr[5] == fr[11] && fr[46] == 0x80 && be16(fr + 16) == 52);
            }
            CHECK(sec, memcmp(t2, &raw[after_at], 32) == 0);
            const uint32_t status = (o.res[1] >> 16) & 0xFFu, flags = o.res[1] >> 24;
            const bool on_list_before = raw[at - 68 + 14] || raw[at - 68 + 15] || n_opts;
            CHECK(sec, ((flags & MTCP_GPU_ACKGEN_ON_LIST) != 0) == on_list_before);
            // it leaves the reference's list iff the record's count and is_wack are 0
            CHECK(sec, listed == (uint32_t)(t2[14] || t2[15]));
            CHECK(sec, status >= MTCP_GPU_ACKGEN_IDLE);
            CHECK(sec, (status == MTCP_GPU_ACKGEN_NO_ROOM) == (listed && n_frames == budget));
        }
        at = after_at + 56;
    }
    if (at != raw.size()) exit(2);
}

void random_cases(Section &sec, long n) {
    for (long c = 0; c < n; ++c) {
        uint8_t tx[32];
        for (int i = 0; i < 32; i += 4) {
            const uint32_t v = rnd();
            memcpy(tx + i, &v, 4);
        }
        const uint32_t n_links = 1 + rnd() % 256;
        if (c & 1) {                                               // the fields of the BAD test made sane
            tx[14] &= 63, tx[15] &= 1, tx[16] &= 31, tx[17] = (uint8_t)(tx[17] % n_links), tx[18] &= 1, tx[19] &= 1;
            memset(tx + 24, 0, 8);
        }
        Walk k = {rnd(), rnd(), rnd(), rnd(), rnd(), rnd()};
        if (rnd() & 1) k.rcv_nxt = k.head_seq + k.merged_len - (rnd() & 3);
        if (rnd() % 4 == 0) k.rcv_wnd >>= rnd() % 33 & 31;
        std::vector<uint32_t> w(rnd() % 200);
        const uint32_t kind = rnd() % 3;
        for (auto &x : w) {
            x = rnd();
            if (kind == 1) x = (x & 0x00FFFFFFu) | (rnd() & 1 ? MTCP_GPU_RCV_ACK_NOW : MTCP_GPU_RCV_ACK_AGGREGATE) << 24;
            if (kind == 2) x = (x & 0x00FFFFFFu) | (rnd() % 8 ? MTCP_GPU_RCV_ACK_NOW : MTCP_GPU_RCV_ACK_AGGREGATE) << 24;
        }
        const bool deferred = rnd() % 4 == 0;
        // the room rule's closed form against the rule record by record, for geometries cut by seg_cap, by
        // buf_len and by the 32-bit descriptor offset
        const uint32_t off_shift = rnd() % 17, a_ = off_shift ? 1u << off_shift : 2u;
        const uint32_t slot = mg::ackgen_slot(off_shift, rnd() & 1 ? 0u : ((66u + rnd() % 300 + a_ - 1) & ~(a_ - 1)));
        const uint32_t seg_cap = 1 + rnd() % 200;
        const uint64_t lim = 0xFFFFFFFFull << off_shift;
        const uint64_t buf_off = (rnd() % 3 == 0 ? lim - (uint64_t)(rnd() % 300) * slot + (rnd() % 3) * a_ - a_
                                                 : (uint64_t)rnd() * a_) & ~(uint64_t)(a_ - 1);
        const uint64_t buf_len = rnd() & 1 ? ~0ull >> 2 : buf_off + rnd() % (uint32_t)(300 * slot) - (rnd() % 3 ? 0 : 70);
        uint32_t by_record = 0;
        while (by_record < seg_cap) {
            const uint64_t at = buf_off + (uint64_t)by_record * slot;
            if (at + 66 > buf_len || (at >> off_shift) > 0xFFFFFFFFull) break;
            by_record++;
        }
        CHECK(sec, slot % a_ == 0 && slot >= 66 && mg::ackgen_room(buf_off, buf_len, off_shift, slot, seg_cap) == by_record);
        const uint32_t S = rnd() % 100, E = rnd() % 200, cur_ts = rnd();
        uint8_t a[32], b[32];
        memcpy(a, tx, 32), memcpy(b, tx, 32);
        Out oa, ob, of;
        host_stream(a, w, false, deferred, k, S, E, cur_ts, n_links, oa);
        host_stream(b, w, true, deferred, k, S, E, cur_ts, n_links, ob);
        sec.cases++;
        CHECK(sec, memcmp(a, b, 32) == 0 && memcmp(oa.res, ob.res, 16) == 0 && oa.recs == ob.recs);
        mg::AckGenTx t;
        memcpy(&t, tx, 32);
        const uint32_t status = (oa.res[1] >> 16) & 0xFFu;
        if (mg::ackgen_bad(t, n_links)) {
            CHECK(sec, status == MTCP_GPU_ACKGEN_BAD && memcmp(a, tx, 32) == 0 && oa.recs.empty());
            CHECK(sec, (c & 1) == 0);
        } else {
            // the fixed bytes: addresses, ports, wscale_mine, link, rsvd
            CHECK(sec, memcmp(a, tx, 12) == 0 && a[16] == tx[16] && a[17] == tx[17] && memcmp(a + 24, tx + 24, 8) == 0);
            CHECK(sec, a[14] <= 63 && a[15] <= 1 && a[18] <= 1 && a[19] <= 1 && a[18] >= tx[18] && a[19] >= tx[19]);
            if (deferred) CHECK(sec, status == MTCP_GPU_ACKGEN_DEFERRED && oa.recs.empty() && a[15] == tx[15]);
            if (oa.recs.empty()) CHECK(sec, memcmp(a + 20, tx + 20, 4) == 0 && rd16(a + 12) == rd16(tx + 12));
            // the emitted records are a prefix of what all the room in the world gives
            uint8_t full[32];
            memcpy(full, tx, 32);
            host_stream(full, w, false, deferred, k, 0, 0xFFFFFFFFu, cur_ts, n_links, of);
            CHECK(sec, oa.recs.size() <= of.recs.size() && of.recs.size() <= 64);
            for (size_t i = 0; i < oa.recs.size() && i < of.recs.size(); ++i) CHECK(sec, oa.recs[i] == of.recs[i]);
            const uint32_t left = S < E ? E - S : 0;
            CHECK(sec, oa.recs.size() == (of.recs.size() < left ? of.recs.size() : left));
            CHECK(sec, (status == MTCP_GPU_ACKGEN_NO_ROOM) == (oa.recs.size() < of.recs.size()));
            CHECK(sec, (uint16_t)(rd16(tx + 12) + oa.recs.size()) == rd16(a + 12));
            CHECK(sec, (oa.res[1] & 0xFFu) + ((oa.res[1] >> 8) & 0xFFu) == oa.recs.size());
        }
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    Section fx{"fixture"}, rn{"random"};
    fixture(fx, argv[1]);
    random_cases(rn, 1000000);
    printf("{\"fixture\": {\"cases\": %ld, \"bad\": %ld, \"first_line\": %d}, "
           "\"random\": {\"cases\": %ld, \"bad\": %ld, \"first_line\": %d}}\n",
           fx.cases, fx.bad, fx.first_line, rn.cases, rn.bad, rn.first_line);
    return fx.bad || rn.bad ? 1 : 0;
}
