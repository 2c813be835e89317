// datagen_step_test.cpp — mtcp_amd/csrc/datagen_step.hpp on the CPU, a stand-alone
// program for g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// (tests/test_datagen_step_rules.py builds and runs it; nothing sanitized is
// loaded into Python).  host_stream below is the kernels' order of calls for
// one stream: the fold, the status, the burst, the commit; row f8's loop between
// the two is a plain while loop here (tcp_out.c:401-443), record by record.
//
//   fixture  every stream of every case of tests/golden/datagen_cases.bin
//            (tests/c/ref_datagen_gen.c has the layout): the records after
//            against the reference's stream after, ret, the frames' count and
//            bytes, the RTO list and the window probe;
//   random   records of random bytes (every second one with the fields of the
//            BAD test made sane) and random flag words: the fold over the
//            masks equals the fold packet by packet, a BAD or BAD_BURST stream
//            changes nothing (but BAD_BURST's on_send_list, the fold's), the
//            fixed bytes never change, and the sanitizers stay silent (no
//            shift goes past the width).
//
// Prints one JSON line: per section the cases, the bad ones and the first bad
// line of this file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../mtcp_amd/csrc/datagen_step.hpp"

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

// One stream's three updated records as the kernels see them.
struct Recs {
    uint8_t snd[128], tx[32], dtx[16], state[64];
};

mg::DataGenIn load(const Recs &r) {
    mg::DataGenIn s{};
    s.sb_off = (uint64_t)rd32(r.dtx + 4) << 32 | rd32(r.dtx), s.sb_base_seq = rd32(r.dtx + 8), s.dflags = rd32(r.dtx + 12);
    memcpy(&s.tx, r.tx, 32);
    s.rcv_nxt = rd32(r.state), s.rcv_wnd = rd32(r.state + 4), s.ts_recent = rd32(r.state + 20), s.rstate = rd32(r.state + 28);
    s.snd_nxt = rd32(r.snd), s.snd_una = rd32(r.snd + 4), s.peer_wnd = rd32(r.snd + 12), s.cwnd = rd32(r.snd + 28);
    s.sb_head_seq = rd32(r.snd + 64), s.sb_len = rd32(r.snd + 68), s.sb_size = rd32(r.snd + 72), s.mss2 = rd32(r.snd + 76);
    s.bits = rd32(r.snd + 80), s.bits2 = rd32(r.snd + 84);
    return s;
}

uint32_t fold_serial(uint32_t on, const std::vector<uint32_t> &w) {
    for (uint32_t x : w) on = mg::datagen_fold(on, x);
    return on;
}
uint32_t fold_masks(uint32_t on, const std::vector<uint32_t> &w) {
    for (size_t base = 0; base < w.size(); base += 64) {
        uint64_t add = 0, rm = 0;
        for (size_t i = base; i < w.size() && i < base + 64; ++i) {
            if (w[i] & MTCP_GPU_ACK_FAST_RTX) add |= 1ull << (i - base);
            if (w[i] & MTCP_GPU_ACK_SEND_LIST_REMOVE) rm |= 1ull << (i - base);
        }
        on = mg::datagen_fold_masks(on, add, rm);
    }
    return on;
}

// Row f8 for one burst with `budget` slots left (tcp_out.c:401-443): the result
// record; payload lengths of the frames in lens.
void f8_loop(const uint32_t b[16], uint64_t payload_bytes, uint32_t budget, uint32_t res[4], std::vector<uint32_t> &lens) {
    const uint32_t mss = b[14] & 0xFFFFu, len = b[9], in_flight = b[10], window = b[11], peer_wnd = b[12];
    const uint64_t po = (uint64_t)b[1] << 32 | b[0];
    res[0] = res[1] = res[2] = res[3] = 0;
    lens.clear();
    if ((b[14] >> 24) || b[15] || mss < 13 || mss - 12 > 1460 + 12 || ((b[14] >> 16) & 0xFFu) >= 3) {
        res[3] = MTCP_GPU_TXS_BAD_BURST;
        return;
    }
    if (po > payload_bytes || len > payload_bytes - po) {
        res[3] = MTCP_GPU_TXS_BAD_PAYLOAD;
        return;
    }
    const uint32_t maxlen = mss - 12;
    uint64_t sent = 0;
    uint32_t stop = 0;
    while (sent < len) {
        const uint64_t left = len - sent, p = left < maxlen ? left : maxlen;
        if (in_flight + sent + p > window) {
            stop = MTCP_GPU_TXS_STOP_WINDOW | (in_flight + sent + p > peer_wnd ? MTCP_GPU_TXS_STOP_PEER_WINDOW : 0u);
            break;
        }
        if (lens.size() >= budget) {
            stop = MTCP_GPU_TXS_STOP_NO_ROOM;
            break;
        }
        lens.push_back((uint32_t)p);
        sent += p;
    }
    res[1] = (uint32_t)lens.size(), res[2] = (uint32_t)sent, res[3] = stop << 8;
}

struct Out {
    uint32_t res[4];
    uint32_t burst[16];
    std::vector<uint32_t> lens;
};

// One stream as the kernels run it.  r: its records, updated.
void host_stream(Recs &r, const std::vector<uint32_t> &w, bool masks, bool host_tail, uint32_t n_links,
                 uint64_t payload_bytes, uint32_t budget, uint32_t cur_ts, Out &o) {
    const mg::DataGenIn s = load(r);
    const bool bad = mg::datagen_bad(s, n_links);
    const uint32_t on_before = s.dflags & 1u;
    uint32_t on = on_before;
    if (!bad) on = masks ? fold_masks(on, w) : fold_serial(on, w);
    const uint32_t status = mg::datagen_status(s, n_links, on, host_tail);
    if (status == MTCP_GPU_DATAGEN_SENT) mg::datagen_burst(s, cur_ts, o.burst);
    else mg::datagen_burst_void(o.burst);
    const bool live = status > MTCP_GPU_DATAGEN_BAD;
    const uint32_t park = mg::datagen_park(status, live ? on_before : 0u, on, live && mg::datagen_window32(s) == 0);
    uint32_t f8[4];
    f8_loop(o.burst, payload_bytes, budget, f8, o.lens);
    const mg::DataGenCommit c = mg::datagen_commit(park, f8, rd32(r.snd), rd32(r.snd + 36), rd32(r.snd + 84),
                                                   rd32(r.tx + 12), rd32(r.tx + 16), rd32(r.tx + 20), cur_ts);
    memcpy(o.res, c.res, 16);
    if (!live) return;
    if (c.st_snd_nxt) memcpy(r.snd, &c.snd_nxt, 4);
    if (c.st_rto) memcpy(r.snd + 40, &c.ts_rto, 4), r.snd[85] = 1;
    if (c.st_id_cnt) memcpy(r.tx + 12, &c.id_cnt, 4);
    if (c.st_misc) memcpy(r.tx + 16, &c.misc, 4);
    if (c.st_ts) memcpy(r.tx + 20, &c.ts_lastack_sent, 4);
    if (c.st_on) r.dtx[12] = (uint8_t)c.on_send_list;
}

// A fixture stream record (88 B) as the three records.
Recs from_fixture(const uint8_t *p) {
    Recs r;
    memset(&r, 0, sizeof r);
    memcpy(r.tx, p, 32);
    const uint32_t w[8] = {rd32(p + 32), rd32(p + 36), rd32(p + 40), rd32(p + 44), rd32(p + 48), rd32(p + 52), rd32(p + 56), rd32(p + 60)};
    memcpy(r.snd, &w[0], 4), memcpy(r.snd + 4, &w[1], 4), memcpy(r.snd + 12, &w[2], 4), memcpy(r.snd + 28, &w[3], 4);
    memcpy(r.snd + 36, &w[4], 4), memcpy(r.snd + 40, &w[5], 4), memcpy(r.snd + 64, &w[6], 4), memcpy(r.snd + 68, &w[7], 4);
    const uint32_t size = 8192;
    memcpy(r.snd + 72, &size, 4);
    const uint16_t mss = rd16(p + 64), eff = (uint16_t)(mss - 12);
    memcpy(r.snd + 76, &mss, 2), memcpy(r.snd + 78, &eff, 2);
    r.snd[80] = 4, r.snd[85] = p[66], r.snd[86] = p[67];
    memcpy(r.state, p + 72, 4), memcpy(r.state + 4, p + 76, 4), memcpy(r.state + 20, p + 80, 4);
    r.state[28] = 4;
    const uint64_t off = rd32(p + 84);
    memcpy(r.dtx, &off, 8), memcpy(r.dtx + 8, &w[6], 4);
    r.dtx[12] = p[68], r.dtx[13] = p[69];
    return r;
}

void fixture(Section &sec, const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    std::vector<uint8_t> raw;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + got);
    fclose(f);
    if (raw.size() < 16 || rd32(&raw[0]) != 0x4E454744u || rd32(&raw[4]) != 1) exit(2);
    const uint32_t cases = rd32(&raw[8]);
    size_t at = 16;
    for (uint32_t c = 0; c < cases; ++c) {
        if (at + 8 > raw.size()) exit(2);
        const uint32_t cur_ts = rd32(&raw[at]), ns = raw[at + 7];
        uint32_t budget = rd16(&raw[at + 4]);
        at += 8;
        std::vector<Recs> recs;
        std::vector<const uint8_t *> data;
        std::vector<uint32_t> offs;
        uint64_t arena = 0;
        for (uint32_t i = 0; i < ns; ++i) {
            if (at + 92 > raw.size()) exit(2);
            recs.push_back(from_fixture(&raw[at]));
            const uint32_t nb = rd32(&raw[at + 88]), off = rd32(&raw[at + 84]);
            data.push_back(&raw[at + 92]), offs.push_back(off);
            if (off + (uint64_t)nb + 3 > arena) arena = off + (uint64_t)nb + 3;
            at += 92 + ((nb + 3) & ~3u);
        }
        for (uint32_t i = 0; i < ns; ++i) {
            if (at + 96 > raw.size()) exit(2);
            const int32_t ret = (int32_t)rd32(&raw[at]);
            const uint32_t nf = rd16(&raw[at + 4]), rto_added = raw[at + 6], wack = raw[at + 7];
            const Recs want = from_fixture(&raw[at + 8]);
            at += 96;
            Out o;
            const uint32_t seq0 = rd32(recs[i].snd), head = rd32(recs[i].snd + 64);
            host_stream(recs[i], {}, false, false, 3, arena, budget, cur_ts, o);
            sec.cases++;
            const uint32_t status = o.res[3] & 0xFFu, flags = (o.res[3] >> 16) & 0xFFu;
            CHECK(sec, memcmp(recs[i].snd, want.snd, 128) == 0 && memcmp(recs[i].tx, want.tx, 32) == 0);
            CHECK(sec, recs[i].dtx[12] == want.dtx[12] && recs[i].dtx[13] == want.dtx[13]);
            const int32_t mine = status == MTCP_GPU_DATAGEN_IDLE ? 0x7FFFFFFF
                                 : status == MTCP_GPU_DATAGEN_SENT ? (int32_t)o.res[1]
                                 : status == MTCP_GPU_DATAGEN_CONTROL_WAIT ? -1
                                 : status == MTCP_GPU_DATAGEN_WINDOW ? -3
                                 : status == MTCP_GPU_DATAGEN_NO_ROOM ? -2 : 0;
            CHECK(sec, mine == ret && status != MTCP_GPU_DATAGEN_BAD && status != MTCP_GPU_DATAGEN_BAD_BURST);
            CHECK(sec, o.lens.size() == nf && o.res[1] == nf);
            CHECK(sec, ((flags & MTCP_GPU_DATAGEN_RTO_ADD) != 0) == (rto_added != 0));
            CHECK(sec, ((flags & MTCP_GPU_DATAGEN_WACK_ENQUEUED) != 0) == (wack != 0));
            uint32_t sent = 0;
            for (uint32_t k = 0; k < nf; ++k) {                    // the frames' payload: the burst's bytes in order
                if (at + 4 > raw.size()) exit(2);
                const uint32_t ln = rd16(&raw[at]);
                const uint8_t *fr = &raw[at + 4];
                if (at + 4 + ln > raw.size()) exit(2);
                const uint32_t p = k < o.lens.size() ? o.lens[k] : 0;
                CHECK(sec, ln == 66 + p);
                const uint64_t po = ((uint64_t)o.burst[1] << 32 | o.burst[0]) + sent;
                CHECK(sec, po == offs[i] + (uint64_t)(seq0 - head) + sent);
                if (ln == 66 + p) CHECK(sec, memcmp(fr + 66, data[i] + (seq0 - head) + sent, p) == 0);
                sent += p;
                at += 4 + ((ln + 3) & ~3u);
            }
            budget -= nf < budget ? nf : budget;
        }
    }
    if (at != raw.size()) exit(2);
}

void random_cases(Section &sec, long n) {
    for (long c = 0; c < n; ++c) {
        Recs r;
        uint8_t *all = reinterpret_cast<uint8_t *>(&r);
        for (size_t i = 0; i < sizeof r; i += 4) {
            const uint32_t v = rnd();
            memcpy(all + i, &v, 4);
        }
        const uint32_t n_links = 1 + rnd() % 256;
        if (c & 1) {                                               // the fields of the BAD test made sane
            r.tx[14] &= 63, r.tx[15] &= 1, r.tx[16] &= 31, r.tx[17] = (uint8_t)(r.tx[17] % n_links), r.tx[18] &= 1, r.tx[19] &= 1;
            memset(r.tx + 24, 0, 8);
            r.dtx[12] &= 1, r.dtx[13] &= 1, r.dtx[14] = r.dtx[15] = 0;
            r.snd[87] = 0, r.snd[82] &= 31;
            if (!rd16(r.snd + 78)) r.snd[78] = 1;
            const uint32_t size = rnd() % ((1u << 30) + 1), len = rnd() % (size + 1);
            memcpy(r.snd + 72, &size, 4), memcpy(r.snd + 68, &len, 4);
            if (rnd() & 1) r.snd[80] = 4, r.state[28] = 4;
            if (rnd() & 1) {                                       // and a plausible buffer around snd_nxt
                const uint32_t head = rd32(r.snd) - rnd() % (len + 2), una = head - rnd() % 100, base = head - rnd() % 1000;
                memcpy(r.snd + 64, &head, 4), memcpy(r.snd + 4, &una, 4), memcpy(r.dtx + 8, &base, 4);
                const uint16_t mss = (uint16_t)(12 + rnd() % 1460);
                memcpy(r.snd + 76, &mss, 2);
                const uint64_t off = rnd() % 4096;
                memcpy(r.dtx, &off, 8);
            }
        }
        std::vector<uint32_t> w(rnd() % 200);
        for (auto &x : w) x = rnd() % 4 ? rnd() & ~(uint32_t)(MTCP_GPU_ACK_FAST_RTX | MTCP_GPU_ACK_SEND_LIST_REMOVE) : rnd();
        const bool host_tail = rnd() % 4 == 0;
        const uint64_t payload_bytes = rnd() & 1 ? ~0ull >> 1 : rnd() % 8192;
        const uint32_t budget = rnd() % 8 ? 1u << 30 : rnd() % 4, cur_ts = rnd();
        Recs a = r, b = r;
        Out oa, ob;
        host_stream(a, w, false, host_tail, n_links, payload_bytes, budget, cur_ts, oa);
        host_stream(b, w, true, host_tail, n_links, payload_bytes, budget, cur_ts, ob);
        sec.cases++;
        CHECK(sec, memcmp(&a, &b, sizeof a) == 0 && memcmp(oa.res, ob.res, 16) == 0 && oa.lens == ob.lens);
        CHECK(sec, fold_serial(r.dtx[12] & 1, w) == fold_masks(r.dtx[12] & 1, w));
        const uint32_t status = oa.res[3] & 0xFFu, flags = (oa.res[3] >> 16) & 0xFFu;
        if (mg::datagen_bad(load(r), n_links)) {
            CHECK(sec, status == MTCP_GPU_DATAGEN_BAD && memcmp(&a, &r, sizeof a) == 0 && oa.lens.empty() && flags == 0);
            continue;
        }
        CHECK(sec, (c & 1) == 1 || status != MTCP_GPU_DATAGEN_BAD);
        // the fixed bytes: everything but snd_nxt, ts_rto, on_rto; ip_id, ack_cnt, is_wack, need_wnd_adv,
        // ts_lastack_sent; on_send_list
        Recs m = a;
        memcpy(m.snd, r.snd, 4), memcpy(m.snd + 40, r.snd + 40, 4), m.snd[85] = r.snd[85];
        memcpy(m.tx + 12, r.tx + 12, 4), m.tx[19] = r.tx[19], memcpy(m.tx + 20, r.tx + 20, 4);
        m.dtx[12] = r.dtx[12];
        CHECK(sec, memcmp(&m, &r, sizeof m) == 0);
        CHECK(sec, a.dtx[12] <= 1 && ((flags & MTCP_GPU_DATAGEN_ON_LIST_AFTER) != 0) == (a.dtx[12] == 1));
        CHECK(sec, ((flags & MTCP_GPU_DATAGEN_ON_LIST_BEFORE) != 0) == ((r.dtx[12] & 1) == 1));
        if (status < MTCP_GPU_DATAGEN_SENT) {                      // nothing but the list membership
            m = a, m.dtx[12] = r.dtx[12];
            if (status == MTCP_GPU_DATAGEN_NO_SNDBUF || status == MTCP_GPU_DATAGEN_EMPTY || status == MTCP_GPU_DATAGEN_BEHIND_HEAD)
                m.tx[14] = r.tx[14];                               // ret 0: the count stays (tcp_out.c:645-649 with ret 0)
            CHECK(sec, memcmp(&m, &r, sizeof m) == 0 && a.tx[14] == r.tx[14] && oa.lens.empty() && oa.res[1] == 0 && oa.res[2] == 0);
        }
        if (status == MTCP_GPU_DATAGEN_BAD_BURST || status == MTCP_GPU_DATAGEN_DEFERRED || status == MTCP_GPU_DATAGEN_CONTROL_WAIT)
            CHECK(sec, a.dtx[12] == fold_serial(r.dtx[12] & 1, w));
        if (status >= MTCP_GPU_DATAGEN_SENT) {
            CHECK(sec, rd32(a.snd) == rd32(r.snd) + oa.res[2] && (uint16_t)(rd16(r.tx + 12) + oa.res[1]) == rd16(a.tx + 12));
            CHECK(sec, (status == MTCP_GPU_DATAGEN_SENT) == (a.dtx[12] == 0));
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
