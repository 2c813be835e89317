/*
 * ref_rtosweep_gen.c — TEST INFRASTRUCTURE ONLY: writes tests/golden/rtosweep_cases.bin
 * with the reference's own retransmission timer (tests/make_rtosweep_golden.py
 * compiles and runs it where the reference's sources are present; nothing of
 * them is copied: timer.c is linked, its headers come in by path).
 *
 * What runs: the reference's own AddtoRTOList, CheckRtmTimeout and HandleRTO
 * (mtcp/src/timer.c:30-60, :363-419, :176-337) on a real RTO store.  The list
 * and event functions HandleRTO ends in (AddtoSendList, AddtoControlList,
 * RaiseErrorEvent, DestroyTCPStream) are the counting stubs of
 * ref_rtosweep_stubs.c, so on_send_list stays what the case set.
 *
 * Per case the driver fills 1 to 16 streams, puts those with on_rto on the RTO
 * list with AddtoRTOList in stream order and calls CheckRtmTimeout once per
 * entry of the case's list of cur_ts values, with a thresh no case reaches.
 * Nothing re-arms a stream, so each fires at most once in a case.  The driver
 * aborts unless every ts_rto - rto_now_ts is in [0, RTO_HASH) when the stream
 * is listed: the range where the wheel and a plain ts_rto test agree.
 *
 * The file: u32 magic 'RTOS', u32 version, u32 cases, u32 0; per case
 *   u8 family; u8 streams; u8 calls; u8 0;
 *   per stream, before: a stream record;
 *   per call: u32 cur_ts; per stream a stream record (the counts and `fired` are
 *     of this call alone).
 * A stream record, 56 B: u32 snd_nxt, snd_una, peer_wnd, cwnd, ssthresh, rto,
 * ts_rto, srtt, rttvar, fss; u16 mss; u8 state, nrtx, max_nrtx, on_rto
 * (on_rto_idx >= 0), has_sndbuf, on_send_list, has_socket, close_reason, fired
 * (the call took it off the RTO list), 0; u8 calls of AddtoSendList,
 * AddtoControlList, RaiseErrorEvent, DestroyTCPStream.  All little-endian.
 *
 * Families: 0 ts_rto at cur_ts - 1, cur_ts and cur_ts + 1, also across the
 * 2^32 wrap; 1 several ticks swept in one call; 2 nrtx 0 to 16 and above, with
 * and without a socket; 3 the rto arithmetic: a zero sum, shifts and sums that
 * wrap to 0; 4 ssthresh above and below its floor with cwnd above and below
 * peer_wnd; 5 on_send_list already 1 and no send buffer; 6 states other than
 * ESTABLISHED (the host's); 7 random mixes.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mtcp.h"
#include "tcp_in.h"
#include "tcp_stream.h"
#include "timer.h"

struct mtcp_config CONFIG;
extern void (*rto_stub_hook)(int which, void *stream);

static uint64_t rng_s = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    rng_s ^= rng_s << 13, rng_s ^= rng_s >> 7, rng_s ^= rng_s << 17;
    return (uint32_t)(rng_s >> 16);
}
static uint32_t below(uint32_t n) { return rnd() % n; }

static FILE *out;
static unsigned n_cases;
static void w32(uint32_t v) { fwrite(&v, 4, 1, out); }
static void w16(uint16_t v) { fwrite(&v, 2, 1, out); }
static void w8(uint8_t v) { fwrite(&v, 1, 1, out); }

#define MAX_STREAMS 16
#define MAX_CALLS 4
static mtcp_manager_t mtcp;

struct spec {
    uint32_t snd_nxt, snd_una, peer_wnd, cwnd, ssthresh, rto, ts_rto, srtt, rttvar, fss;
    uint16_t mss;
    uint8_t state, nrtx, max_nrtx, on_rto, has_sndbuf, on_send_list, has_socket;
};

struct live {
    tcp_stream st;
    struct tcp_recv_vars rv;
    struct tcp_send_vars sv;
    struct tcp_send_buffer sb;
    uint8_t calls[4];
};
static struct live lv[MAX_STREAMS];

static void hook(int which, void *stream)
{
    for (unsigned i = 0; i < MAX_STREAMS; ++i)
        if (stream == (void *)&lv[i].st) {
            lv[i].calls[which]++;
            return;
        }
    abort();
}

static void write_record(const struct live *k, int fired)
{
    const tcp_stream *st = &k->st;
    w32(st->snd_nxt), w32(k->sv.snd_una), w32(k->sv.peer_wnd), w32(k->sv.cwnd), w32(k->sv.ssthresh);
    w32(k->sv.rto), w32(k->sv.ts_rto), w32(k->rv.srtt), w32(k->rv.rttvar), w32(k->sv.fss);
    w16(k->sv.mss), w8(st->state), w8(k->sv.nrtx), w8(k->sv.max_nrtx), w8(st->on_rto_idx >= 0);
    w8(k->sv.sndbuf != NULL), w8(k->sv.on_send_list), w8(st->socket != NULL), w8(st->close_reason);
    w8((uint8_t)fired), w8(0);
    w8(k->calls[0]), w8(k->calls[1]), w8(k->calls[2]), w8(k->calls[3]);
}

/* an ESTABLISHED stream on the RTO list with data in flight */
static struct spec base(uint32_t ts_rto)
{
    struct spec s;
    memset(&s, 0, sizeof(s));
    s.snd_una = rnd(), s.snd_nxt = s.snd_una + 1 + below(100000);
    s.mss = below(2) ? 1460 : (uint16_t)(13 + below(1448));
    s.peer_wnd = below(1u << 20), s.cwnd = below(1u << 20), s.ssthresh = rnd();
    s.rto = 1 + below(3000), s.ts_rto = ts_rto;
    s.srtt = below(1u << 16), s.rttvar = below(1u << 12);
    s.state = TCP_ST_ESTABLISHED, s.nrtx = (uint8_t)below(4), s.max_nrtx = (uint8_t)below(4);
    s.on_rto = 1, s.has_sndbuf = 1, s.on_send_list = (uint8_t)below(2), s.has_socket = (uint8_t)below(2);
    return s;
}

static void run_case(int fam, const struct spec *sp, unsigned n, const uint32_t *ts, unsigned calls)
{
    if (n < 1 || n > MAX_STREAMS || calls < 1 || calls > MAX_CALLS || mtcp->rto_list_cnt) abort();
    w8((uint8_t)fam), w8((uint8_t)n), w8((uint8_t)calls), w8(0);
    for (unsigned i = 0; i < n; ++i) {
        const struct spec *s = &sp[i];
        struct live *k = &lv[i];
        memset(k, 0, sizeof(*k));
        tcp_stream *st = &k->st;
        st->rcvvar = &k->rv, st->sndvar = &k->sv;
        st->id = i, st->state = s->state, st->on_rto_idx = -1;
        st->snd_nxt = s->snd_nxt, st->socket = s->has_socket ? (void *)&k->sb : NULL;
        k->sv.snd_una = s->snd_una, k->sv.peer_wnd = s->peer_wnd, k->sv.cwnd = s->cwnd, k->sv.ssthresh = s->ssthresh;
        k->sv.rto = s->rto, k->sv.ts_rto = s->ts_rto, k->sv.fss = s->fss, k->sv.mss = s->mss;
        k->sv.nrtx = s->nrtx, k->sv.max_nrtx = s->max_nrtx;
        k->sv.sndbuf = s->has_sndbuf ? &k->sb : NULL, k->sv.on_send_list = s->on_send_list;
        k->rv.srtt = s->srtt, k->rv.rttvar = s->rttvar;
        if (s->on_rto) {
            AddtoRTOList(mtcp, st);
            /* timer.c:47-52: inside the wheel, the range where it agrees with a plain ts_rto test */
            const int32_t diff = (int32_t)(s->ts_rto - mtcp->rto_store->rto_now_ts);
            if (diff < 0 || diff >= RTO_HASH || st->on_rto_idx < 0 || st->on_rto_idx >= RTO_HASH) abort();
        }
        write_record(k, 0);
    }
    for (unsigned c = 0; c < calls; ++c) {
        uint8_t before[MAX_STREAMS];
        for (unsigned i = 0; i < n; ++i) before[i] = lv[i].st.on_rto_idx >= 0, memset(lv[i].calls, 0, 4);
        if (c && (int32_t)(ts[c] - ts[c - 1]) < 0) abort();
        CheckRtmTimeout(mtcp, ts[c], 1 << 20);
        w32(ts[c]);
        for (unsigned i = 0; i < n; ++i) write_record(&lv[i], before[i] && lv[i].st.on_rto_idx < 0);
    }
    for (unsigned i = 0; i < n; ++i)
        if (lv[i].st.on_rto_idx >= 0) RemoveFromRTOList(mtcp, &lv[i].st);
    n_cases++;
}

static void one(int fam, struct spec s) { run_case(fam, &s, 1, &s.ts_rto, 1); }

int main(int argc, char **argv)
{
    if (argc < 2 || !(out = fopen(argv[1], "wb"))) return 2;
    mtcp = calloc(1, sizeof(*mtcp));
    mtcp->rto_store = InitRTOHashstore();
    if (!mtcp->rto_store) abort();
    rto_stub_hook = hook;
    w32(0x534F5452u), w32(1), w32(0), w32(0);                     /* 'RTOS' */

    struct spec l[MAX_STREAMS];
    {                                                             /* 0: around cur_ts */
        const uint32_t T[6] = {1000, 0, 1, 0xFFFFFFFFu, 0xFFFFFFFEu, 0x80000000u};
        for (unsigned i = 0; i < 6; ++i) {
            l[0] = base(T[i] - 1), l[1] = base(T[i]), l[2] = base(T[i] + 1), l[3] = base(T[i]);
            l[3].on_rto = 0;                                      /* not on the list: never fires */
            const uint32_t ts[3] = {T[i], T[i], T[i] + 1};
            run_case(0, l, 4, ts, 3);
        }
    }
    for (unsigned i = 0; i < 6; ++i) {                            /* 1: several ticks in one call */
        const uint32_t T = i < 3 ? rnd() : 0xFFFFFFFFu - below(40);
        const uint32_t d[8] = {0, 1, 5, 5, 40, 2999, 17, 6};
        for (unsigned j = 0; j < 8; ++j) l[j] = base(T + d[j]);
        const uint32_t ts[4] = {T + 5, T + 39, T + 40, T + 3500};
        run_case(1, l, 8, ts, 4);
    }
    for (unsigned nr = 0; nr <= 19; ++nr)                         /* 2: the count, the backoff cap, the LOST exit */
        for (unsigned sock = 0; sock < 2; ++sock) {
            struct spec s = base(rnd());
            s.nrtx = nr < 18 ? (uint8_t)nr : nr == 18 ? 200 : 255, s.max_nrtx = (uint8_t)below(20), s.has_socket = (uint8_t)sock;
            one(2, s);
        }
    {                                                             /* 3: the rto arithmetic */
        const uint32_t sv[8][3] = {{7, 0, 0},           {0, 0, 5},          {0x10000000u, 0, 5}, {0x10000000u, 0, 6},
                                   {0, 0x80000000u, 0}, {8, 0xFFFFFFFFu, 2}, {0, 0x02000000u, 9}, {0xFFFFFFFFu, 0xFFFFFFFFu, 3}};
        for (unsigned i = 0; i < 8; ++i) {
            struct spec s = base(rnd());
            s.srtt = sv[i][0], s.rttvar = sv[i][1], s.nrtx = (uint8_t)sv[i][2];
            one(3, s);
        }
    }
    {                                                             /* 4: ssthresh and its floor */
        const uint16_t mss[4] = {536, 1460, 65535, 0};
        for (unsigned i = 0; i < 32; ++i) {
            struct spec s = base(rnd());
            s.mss = mss[i % 4];
            const uint32_t floor2 = 2u * s.mss, lo = (i & 4) ? 2 * floor2 + 2 + below(9000) : below(2 * floor2 + 1);
            if (i & 8) s.cwnd = lo, s.peer_wnd = lo + below(5000);
            else s.peer_wnd = lo, s.cwnd = lo + 1 + below(5000);
            if (i & 16) s.cwnd = s.peer_wnd = 2 * floor2 + (i & 1);    /* the quotient at the floor and one below */
            one(4, s);
        }
    }
    for (unsigned i = 0; i < 8; ++i) {                            /* 5: the send list */
        struct spec s = base(rnd());
        s.on_send_list = (uint8_t)(i & 1), s.has_sndbuf = (uint8_t)((i >> 1) & 1), s.nrtx = i & 4 ? 16 : 2;
        one(5, s);
    }
    {                                                             /* 6: the host's states */
        const uint8_t stt[10] = {TCP_ST_SYN_SENT, TCP_ST_SYN_SENT,   TCP_ST_SYN_RCVD, TCP_ST_CLOSE_WAIT, TCP_ST_FIN_WAIT_1,
                                 TCP_ST_FIN_WAIT_1, TCP_ST_CLOSING, TCP_ST_LAST_ACK, TCP_ST_FIN_WAIT_2, TCP_ST_SYN_RCVD};
        const uint8_t nr[10] = {3, 7, 6, 1, 2, 2, 0, 5, 1, 16};
        for (unsigned i = 0; i < 10; ++i)
            for (unsigned sock = 0; sock < 2; ++sock) {
                struct spec s = base(rnd());
                s.state = stt[i], s.nrtx = nr[i], s.has_socket = (uint8_t)sock;
                s.fss = i == 4 ? s.snd_una + 10 : s.snd_una;      /* data before the FIN, or the FIN itself */
                one(6, s);
            }
    }
    for (unsigned i = 0; i < 40; ++i) {                           /* 7: random mixes */
        const unsigned n = 1 + below(MAX_STREAMS);
        const uint32_t T = i % 5 == 4 ? 0xFFFFFFFFu - below(100) : rnd();
        for (unsigned j = 0; j < n; ++j) {
            l[j] = base(T + (j ? below(200) : 0));                /* the first listed stream sets rto_now_ts */
            l[j].nrtx = (uint8_t)below(19);
            if (below(8) == 0) l[j].on_rto = 0;
            if (below(8) == 0) l[j].has_sndbuf = 0;
            if (below(6) == 0) l[j].state = (uint8_t)(below(2) ? TCP_ST_CLOSE_WAIT : TCP_ST_SYN_RCVD);
            if (below(6) == 0) l[j].srtt = rnd(), l[j].rttvar = rnd();
        }
        l[0].on_rto = 1;
        uint32_t t2[4];
        t2[0] = T + below(60), t2[1] = t2[0] + below(80), t2[2] = t2[1] + below(80), t2[3] = t2[2] + 400;
        run_case(7, l, n, t2, 4);
    }
    fseek(out, 8, SEEK_SET);
    w32(n_cases);
    fclose(out);
    printf("%u cases\n", n_cases);
    return 0;
}
