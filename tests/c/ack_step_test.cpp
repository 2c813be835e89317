// ack_step_test.cpp — mtcp_amd/csrc/ack_step.hpp on the CPU, a stand-alone
// program for g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// (tests/test_ack_step_rules.py builds and runs it; nothing sanitized is loaded
// into Python).
//
//   fixture  ack_step over every walk of tests/golden/ackwalk_cases.bin
//            (tests/c/ref_ackwalk_gen.c has the layout): after every packet
//            the 18 state words, dup_acks, nrtx, on_rto, the bytes that left
//            the send buffer and the reference's call counts against the
//            record's flags;
//   random   ack_step over states and inputs of random bytes (every second
//            state with the fields of the BAD test made sane, so that the
//            arithmetic is reached): a deferred packet changes no byte, a
//            walked one none of the fixed bytes, and the sanitizers stay
//            silent: signed overflow and division by zero are what
//            DEFER_ARITH has fenced off.
//
// Prints one JSON line: per section the cases, the bad ones and the first bad
// line of this file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../mtcp_amd/csrc/ack_step.hpp"

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

void fixture(Section &sec, const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        CHECK(sec, false);
        return;
    }
    std::vector<uint8_t> raw(1 << 20);
    const size_t got = fread(raw.data(), 1, raw.size(), f);
    fclose(f);
    raw.resize(got);                                  // exact size: a read past the end is a report
    CHECK(sec, got >= 16 && rd32(&raw[0]) == 0x574B4341u && rd32(&raw[4]) == 1 && rd32(&raw[12]) == 16);
    if (sec.bad) return;
    const uint32_t walks = rd32(&raw[8]);
    size_t off = 16;
    for (uint32_t w = 0; w < walks; ++w) {
        mg::AckState s;
        memcpy(&s, &raw[off], sizeof(s));
        const uint32_t npkt = rd32(&raw[off + 92]);
        off += 96;
        bool deferred = false;
        for (uint32_t i = 0; i < npkt; ++i, off += 112) {
            const uint8_t *p = &raw[off];
            const uint32_t cur_ts = rd32(p + 12), window = rd16(p + 16), len = rd16(p + 18);
            const uint32_t has_ack = p[20], has_ts = p[21], ret = p[22];
            uint32_t bits = len == 0 ? mg::kAckInNoPayload : 0u;
            if (ret) bits |= mg::kAckInValid;
            if (has_ts) bits |= mg::kAckInHasTs;
            uint4 in;
            in.x = rd32(p), in.y = rd32(p + 4), in.z = rd32(p + 8);
            in.w = window | (has_ack ? 0x10u : 0u) << 16 | bits << 24;
            const mg::AckState before = s;
            const uint4 r = mg::ack_step(s, in, cur_ts, deferred);
            const uint32_t flags = r.w & 0xFFFFu, verdict = (r.w >> 16) & 0xFFu;
            sec.cases++;
            CHECK(sec, !deferred && verdict >= MTCP_GPU_ACK_NOT_VALID);
            CHECK(sec, memcmp(&s, p + 36, 72) == 0);                       // the 18 words
            CHECK(sec, (s.bits >> 24) == p[108] && (s.bits2 & 0xFFu) == p[109] && ((s.bits2 >> 8) & 0xFFu) == p[110]);
            CHECK(sec, s.sb_size == before.sb_size && s.mss2 == before.mss2 &&
                           (s.bits & 0xFFFFFFu) == (before.bits & 0xFFFFFFu) && (s.bits2 >> 16) == (before.bits2 >> 16));
            CHECK(sec, r.x == rd32(p + 32));
            CHECK(sec, p[24] == !!(flags & MTCP_GPU_ACK_WRITE_EVENT_WND) && p[25] == !!(flags & MTCP_GPU_ACK_WRITE_EVENT_ROOM));
            CHECK(sec, p[26] == !!(flags & MTCP_GPU_ACK_FAST_RTX) && p[27] == !!(flags & MTCP_GPU_ACK_SEND_LIST_REMOVE));
            CHECK(sec, p[28] == !!(flags & MTCP_GPU_ACK_RTO_REMOVE) && p[29] == !!(flags & MTCP_GPU_ACK_RTO_ADD));
            CHECK(sec, r.y == s.snd_nxt && r.z == s.cwnd && (r.w >> 24) == (s.bits >> 24));
            CHECK(sec, (verdict == MTCP_GPU_ACK_NOT_VALID) == !ret);
            CHECK(sec, mg::ack_dirty(r) != 0 || memcmp(&s, &before, sizeof(s)) == 0);
        }
    }
    CHECK(sec, off == raw.size() && sec.cases == 16L * walks);
}

void random_bytes(Section &sec, long steps) {
    long walked = 0, arith = 0, fresh = 0;
    for (long c = 0; c < steps; ++c) {
        uint32_t w[22];
        for (uint32_t &x : w) x = rnd();
        mg::AckState s;
        memcpy(&s, w, sizeof(s));
        if (c & 1) {                                  // passes the BAD test; ESTABLISHED; small or random words
            const uint32_t size = 1u << (10 + rnd() % 21);
            s.sb_size = size, s.sb_len = rnd() % (size + 1);
            if ((s.mss2 >> 16) == 0) s.mss2 |= 1u << 16;
            s.bits = MTCP_GPU_ACK_ST_ESTABLISHED | (rnd() & 0xFF00u) | (rnd() % 32) << 16 | (rnd() & 0xFFu) << 24;
            s.bits2 &= 0x00FFFFFFu;
            if (c & 2) s.snd_nxt = s.sb_head_seq + s.sb_len, s.snd_una = s.last_ack_seq = s.sb_head_seq;
            if (c & 4) s.cwnd = rnd() % 4 ? rnd() % 100000 : 0, s.ssthresh = rnd() % 100000;
            if (c & 32) s.srtt = 0;                   // no estimate yet
        }
        const uint32_t cur_ts = rnd();
        bool deferred = false;
        for (int k = 0; k < 4; ++k) {                 // a few packets on the same state
            uint4 in;
            in.x = rnd(), in.y = (c & 8) ? s.sb_head_seq + (uint32_t)(rnd() % ((uint64_t)s.sb_len + 2000u)) - 1000u : rnd(), in.z = rnd();
            in.w = rnd();
            if (c & 16) in.w = (in.w & 0x00F8FFFFu) | 0x00100000u | (mg::kAckInValid | mg::kAckInHasTs | (rnd() & 1u)) << 24;
            const mg::AckState before = s;
            const bool was = deferred;
            const uint4 r = mg::ack_step(s, in, cur_ts, deferred);
            const uint32_t verdict = (r.w >> 16) & 0xFFu;
            sec.cases++;
            CHECK(sec, verdict >= MTCP_GPU_ACK_DEFER_RCV && verdict <= MTCP_GPU_ACK_ACK_NEW);
            CHECK(sec, deferred == (verdict <= MTCP_GPU_ACK_DEFER_BEHIND) && (!was || verdict == MTCP_GPU_ACK_DEFER_BEHIND));
            if (deferred) CHECK(sec, memcmp(&s, &before, sizeof(s)) == 0 && r.x == 0 && r.y == 0 && r.z == 0 && (r.w & 0xFF00FFFFu) == 0);
            CHECK(sec, s.sb_size == before.sb_size && s.mss2 == before.mss2 &&
                           (s.bits & 0xFFFFFFu) == (before.bits & 0xFFFFFFu) && (s.bits2 >> 16) == (before.bits2 >> 16));
            CHECK(sec, mg::ack_dirty(r) != 0 || memcmp(&s, &before, sizeof(s)) == 0);
            if (!(mg::ack_dirty(r) & 2u)) CHECK(sec, memcmp(&s.ssthresh, &before.ssthresh, 48) == 0);
            walked += verdict == MTCP_GPU_ACK_ACK_NEW, arith += verdict == MTCP_GPU_ACK_DEFER_ARITH;
            fresh += verdict == MTCP_GPU_ACK_ACK_NEW && before.srtt == 0 && ((before.bits >> 8) & 0xFFu);
        }
    }
    if (getenv("ACK_STEP_TEST_COUNTS")) fprintf(stderr, "walked %ld arith %ld fresh %ld\n", walked, arith, fresh);
    CHECK(sec, walked > steps / 50 && arith > steps / 2000 && fresh > 0);     // the arithmetic was reached
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s FIXTURE\n", argv[0]);
        return 2;
    }
    Section fix{"fixture"}, ran{"random"};
    fixture(fix, argv[1]);
    random_bytes(ran, 500000);
    printf("{\"%s\": {\"cases\": %ld, \"bad\": %ld, \"first_line\": %d}, \"%s\": {\"cases\": %ld, \"bad\": %ld, \"first_line\": %d}}\n",
           fix.name, fix.cases, fix.bad, fix.first_line, ran.name, ran.cases, ran.bad, ran.first_line);
    return fix.bad || ran.bad ? 1 : 0;
}
