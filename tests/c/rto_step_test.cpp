// rto_step_test.cpp — mtcp_amd/csrc/rto_step.hpp on the CPU, a stand-alone
// program for g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined
// (tests/test_rto_step_rules.py builds and runs it; nothing sanitized is loaded
// into Python).
//
//   fixture  rto_due and rto_step over every stream of every CheckRtmTimeout
//            call of tests/golden/rtosweep_cases.bin (tests/c/ref_rtosweep_gen.c
//            has the layout): the due test against `fired`; for a fired
//            ESTABLISHED stream nrtx, rto, ssthresh, cwnd, snd_nxt, state,
//            on_rto and the reference's call counts against the step's stores,
//            verdict and flags; any other fired stream is DEFER_STATE with no
//            store;
//   random   rto_step over records of random bytes (every second one with the
//            fields of the BAD test made sane, every tcp_state, any nrtx)
//            against a second, literal restatement of the header's contract
//            on whole records: every byte of both records and the result.
//
// Prints one JSON line: per section the cases, the bad ones and the first bad
// line of this file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../mtcp_amd/csrc/rto_step.hpp"

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

// The step over whole records, as the sweep kernel applies it: loads, rto_step,
// the stores RtoOut names.  Returns dwords 1-3 of the result record.
void apply(mtcp_gpu_ack_state &s, mtcp_gpu_datagen_state &d, uint32_t rec[3]) {
    uint32_t w[22], dw[4];
    memcpy(w, &s, 88);
    memcpy(dw, &d, 16);
    mg::RtoIn in;
    in.snd_una = w[1], in.peer_wnd = w[3], in.cwnd = w[7], in.rto = w[9], in.srtt = w[11], in.rttvar = w[14];
    in.sb_len = w[17], in.sb_size = w[18], in.mss2 = w[19], in.bits = w[20], in.bits2 = w[21], in.dflags = dw[3];
    const mg::RtoOut o = mg::rto_step(in);
    if (o.st_win) w[0] = o.snd_nxt, w[7] = o.cwnd, w[8] = o.ssthresh, w[9] = o.rto;
    if (o.st_bits) w[20] = o.bits, w[21] = o.bits2;
    memcpy(&s, w, 88);
    if (o.st_on) d.on_send_list = 1;
    memcpy(rec, o.rec, 12);
}

// The header's contract once more, on the struct's fields.
void restated(mtcp_gpu_ack_state &s, mtcp_gpu_datagen_state &d, mtcp_gpu_rto_rec &r) {
    memset(&r, 0, sizeof(r));
    r.rto = s.rto, r.nrtx = s.nrtx;
    const bool snd_bad = s.rsvd != 0 || s.eff_mss == 0 || s.wscale_peer > 31 || s.sb_size > (1u << 30) || s.sb_len > s.sb_size;
    const bool dtx_bad = d.rsvd[0] || d.rsvd[1] || d.on_send_list > 1 || d.on_control_list > 1;
    if (snd_bad || dtx_bad) {
        r.verdict = MTCP_GPU_RTO_BAD;
        return;
    }
    if (s.tcp_state != 4) {
        r.verdict = MTCP_GPU_RTO_DEFER_STATE;
        return;
    }
    if (s.nrtx >= 16) {
        r.verdict = MTCP_GPU_RTO_LOST;
        s.on_rto = 0, s.tcp_state = 0;
        return;
    }
    r.verdict = MTCP_GPU_RTO_RETRANSMIT;
    s.on_rto = 0;
    s.nrtx = (uint8_t)(s.nrtx + 1);
    const unsigned backoff = s.nrtx < 7 ? s.nrtx : 7;
    const uint32_t rto = (uint32_t)((uint64_t)(uint32_t)((s.srtt >> 3) + s.rttvar) << backoff);
    if (rto) s.rto = rto;
    uint32_t half = (s.cwnd < s.peer_wnd ? s.cwnd : s.peer_wnd) / 2;
    if (half < 2u * s.mss) half = 2u * s.mss;
    s.ssthresh = half;
    s.cwnd = s.mss;
    s.snd_nxt = s.snd_una;
    if (s.has_sndbuf) {
        if (!d.on_send_list) r.flags |= MTCP_GPU_RTO_SEND_LIST_ADD;
        d.on_send_list = 1;
    }
    r.rto = s.rto, r.nrtx = s.nrtx;
}

// One 56 B stream record of the fixture.
struct FixRec {
    uint32_t snd_nxt, snd_una, peer_wnd, cwnd, ssthresh, rto, ts_rto, srtt, rttvar, fss;
    uint16_t mss;
    uint8_t state, nrtx, max_nrtx, on_rto, has_sndbuf, on_send_list, has_socket, close_reason, fired, pad;
    uint8_t calls[4];
};
FixRec fix_rec(const uint8_t *p) {
    FixRec r;
    uint32_t *w = &r.snd_nxt;
    for (int i = 0; i < 10; ++i) w[i] = rd32(p + 4 * i);
    r.mss = rd16(p + 40);
    memcpy(&r.state, p + 42, 14);
    return r;
}

void mirror(const FixRec &f, mtcp_gpu_ack_state &s, mtcp_gpu_datagen_state &d) {
    memset(&s, 0, sizeof(s)), memset(&d, 0, sizeof(d));
    s.snd_nxt = f.snd_nxt, s.snd_una = f.snd_una, s.peer_wnd = f.peer_wnd, s.cwnd = f.cwnd, s.ssthresh = f.ssthresh;
    s.rto = f.rto, s.ts_rto = f.ts_rto, s.srtt = f.srtt, s.rttvar = f.rttvar, s.mss = f.mss;
    s.eff_mss = f.mss > 12 ? (uint16_t)(f.mss - 12) : 1;
    s.sb_len = 4000, s.sb_size = 8192, s.tcp_state = f.state, s.nrtx = f.nrtx, s.on_rto = f.on_rto;
    s.has_sndbuf = f.has_sndbuf;
    d.on_send_list = f.on_send_list;
}

void fixture(Section &sec, const char *path) {
    FILE *fp = fopen(path, "rb");
    if (!fp) {
        CHECK(sec, false);
        return;
    }
    std::vector<uint8_t> raw;
    uint8_t buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof(buf), fp)) > 0;) raw.insert(raw.end(), buf, buf + k);
    fclose(fp);
    CHECK(sec, raw.size() >= 16 && rd32(&raw[0]) == 0x534F5452u && rd32(&raw[4]) == 1);
    if (sec.bad) return;
    const uint32_t cases = rd32(&raw[8]);
    size_t at = 16;
    for (uint32_t c = 0; c < cases; ++c) {
        const unsigned ns = raw.at(at + 1), nc = raw.at(at + 2);
        at += 4;
        std::vector<mtcp_gpu_ack_state> snd(ns);
        std::vector<mtcp_gpu_datagen_state> dtx(ns);
        std::vector<FixRec> before(ns);
        for (unsigned i = 0; i < ns; ++i, at += 56) {
            (void)raw.at(at + 55);
            before[i] = fix_rec(&raw[at]);
            mirror(before[i], snd[i], dtx[i]);
        }
        for (unsigned k = 0; k < nc; ++k) {
            (void)raw.at(at + 3);
            const uint32_t cur_ts = rd32(&raw[at]);
            at += 4;
            for (unsigned i = 0; i < ns; ++i, at += 56) {
                (void)raw.at(at + 55);
                const FixRec a = fix_rec(&raw[at]);
                sec.cases++;
                uint32_t w21;
                memcpy(&w21, reinterpret_cast<const uint8_t *>(&snd[i]) + 84, 4);
                const bool due = mg::rto_due(w21, snd[i].ts_rto, cur_ts);
                CHECK(sec, due == (a.fired != 0));
                if (!due) continue;
                const mtcp_gpu_ack_state s0 = snd[i];
                const mtcp_gpu_datagen_state d0 = dtx[i];
                uint32_t rec[3];
                apply(snd[i], dtx[i], rec);
                const uint32_t verdict = (rec[1] >> 8) & 0xFFu, flags = (rec[1] >> 16) & 0xFFu;
                if (s0.tcp_state != 4) {                      // the host's: nothing changes, then the host refreshes
                    CHECK(sec, verdict == MTCP_GPU_RTO_DEFER_STATE && !memcmp(&s0, &snd[i], 128) && !memcmp(&d0, &dtx[i], 16));
                    snd[i].on_rto = 0;
                    continue;
                }
                CHECK(sec, snd[i].nrtx == a.nrtx && snd[i].rto == a.rto && snd[i].tcp_state == a.state && snd[i].on_rto == a.on_rto);
                CHECK(sec, rec[0] == a.rto && (rec[1] & 0xFFu) == a.nrtx && rec[2] == 0);
                if (s0.nrtx >= 16) {
                    CHECK(sec, verdict == MTCP_GPU_RTO_LOST && a.close_reason == 4 && a.calls[2] + a.calls[3] == 1 && !a.calls[0]);
                    CHECK(sec, snd[i].ssthresh == a.ssthresh && snd[i].cwnd == a.cwnd && snd[i].snd_nxt == a.snd_nxt && !flags);
                    CHECK(sec, dtx[i].on_send_list == d0.on_send_list);
                } else {
                    CHECK(sec, verdict == MTCP_GPU_RTO_RETRANSMIT && a.calls[0] == 1 && !a.calls[1] && !a.calls[2] && !a.calls[3]);
                    CHECK(sec, snd[i].ssthresh == a.ssthresh && snd[i].cwnd == a.cwnd && snd[i].snd_nxt == a.snd_nxt);
                    CHECK(sec, snd[i].snd_una == a.snd_una && snd[i].ts_rto == a.ts_rto && snd[i].peer_wnd == a.peer_wnd);
                    CHECK(sec, dtx[i].on_send_list == (s0.has_sndbuf ? 1 : d0.on_send_list));
                    CHECK(sec, (flags == MTCP_GPU_RTO_SEND_LIST_ADD) == (s0.has_sndbuf && !d0.on_send_list) && flags <= 1);
                }
            }
        }
    }
    CHECK(sec, at == raw.size());
}

void random_records(Section &sec, long n) {
    for (long t = 0; t < n; ++t) {
        mtcp_gpu_ack_state s;
        mtcp_gpu_datagen_state d;
        uint32_t w[36];
        for (int i = 0; i < 32; ++i) w[i] = rnd();
        for (int i = 32; i < 36; ++i) w[i] = rnd();
        memcpy(&s, w, 128), memcpy(&d, w + 32, 16);
        if (t & 1) {                                          // past the BAD test
            s.rsvd = 0, s.eff_mss |= 1, s.wscale_peer &= 31, s.sb_size &= (1u << 30) - 1;
            s.sb_len = s.sb_size ? s.sb_len % s.sb_size : 0;
            d.rsvd[0] = d.rsvd[1] = 0, d.on_send_list &= 1, d.on_control_list &= 1;
            if (t & 2) s.tcp_state = 4;
            if (t & 4) s.nrtx = (uint8_t)(rnd() % 19);
            if (t & 8) s.srtt = rnd() % 9, s.rttvar = (t & 16) ? 0u - (s.srtt >> 3) : 0x02000000u;
        }
        mtcp_gpu_ack_state s1 = s, s2 = s;
        mtcp_gpu_datagen_state d1 = d, d2 = d;
        uint32_t rec[3];
        mtcp_gpu_rto_rec want;
        apply(s1, d1, rec);
        restated(s2, d2, want);
        sec.cases++;
        CHECK(sec, !memcmp(&s1, &s2, 128) && !memcmp(&d1, &d2, 16));
        CHECK(sec, !memcmp(reinterpret_cast<const uint8_t *>(&s1) + 88, reinterpret_cast<const uint8_t *>(&s) + 88, 40));
        uint32_t ww[4];
        memcpy(ww, &want, 16);
        CHECK(sec, ww[0] == 0 && rec[0] == ww[1] && rec[1] == ww[2] && rec[2] == ww[3]);
        if (want.verdict <= MTCP_GPU_RTO_DEFER_STATE) CHECK(sec, !memcmp(&s1, &s, 128) && !memcmp(&d1, &d, 16));
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    Section fx{"fixture"}, rn{"random"};
    fixture(fx, argv[1]);
    random_records(rn, 2000000);
    printf("{\"fixture\": {\"cases\": %ld, \"bad\": %ld, \"first_line\": %d}, "
           "\"random\": {\"cases\": %ld, \"bad\": %ld, \"first_line\": %d}}\n",
           fx.cases, fx.bad, fx.first_line, rn.cases, rn.bad, rn.first_line);
    return fx.bad || rn.bad ? 1 : 0;
}
