/*
 * ref_ackgen_gen.c — TEST INFRASTRUCTURE ONLY: writes tests/golden/ackgen_cases.bin
 * with the reference's own ACK sending (tests/make_ackgen_golden.py compiles and
 * runs it where the reference's sources are present; nothing of them is copied:
 * tcp_out.c comes in by path, which makes its static GenerateTCPOptions and its
 * inline EnqueueACK, AddtoACKList, WriteTCPACKList and SendTCPPacket reachable).
 *
 * Which output path runs: the reference's own IPOutput (ip_out.c, linked) and
 * its own EthernetOutput (eth_out.c, linked), with counting stand-ins in this
 * file for GetDestinationHWaddr, RequestARP and UpdateTimeoutList
 * (GetOutputInterface is ip_out.c's own and is never reached: nif_out is
 * always set), against this file's slot source: an io_module whose
 * get_wptr hands out 66 B slots and runs dry after r of them.  tcp_util.c is
 * linked for TCPCalcChecksum.
 *
 * Per case the driver fills a stream, calls EnqueueACK once per option of the
 * case, then WriteTCPACKList once, and aborts if a field the tx record calls
 * fixed has changed, if snd_nxt or the RTO list was touched, or if
 * UpdateTimeoutList was not called once per frame.
 *
 * The file: u32 magic 'ACKG', u32 version, u32 cases, u32 0; per case
 *   before:  the 32 B of struct mtcp_gpu_ackgen_state (include/mtcp_gpu_ackgen.h),
 *            then u32 snd_nxt, rcv_nxt, rcv_wnd, head_seq, merged_len, ts_recent;
 *   u32 cur_ts; u16 the slot budget r; u16 options; u16 frames; u8 family;
 *   u8 on_ack_list after;
 *   the options, one byte each (ACK_OPT_NOW 0, ACK_OPT_AGGREGATE 1, ACK_OPT_WACK 2,
 *   tcp_out.h:9-14), padded with 0xFF to a multiple of 4;
 *   the frames written, 66 B each;
 *   after:   as before.
 * has_rcvbuf is rcvvar->rcvbuf != NULL; link is sndvar->nif_out, the Ethernet
 * addresses being 02:00:00:00:00:<link> (the ARP answer) and 02:01:00:00:00:<link>
 * (CONFIG.eths[].haddr).  All little-endian.
 *
 * Families: 0 AGGREGATE only; 1 k NOWs, k = 1..70; 2 mixed sequences with a
 * count on entry; 3 is_wack with and without plain ACKs; 4 rcvbuf == NULL;
 * 5 rcv_nxt past head_seq + merged_len; 6 a slot budget that cuts inside the
 * plain ACKs, in front of the probe, and at 0; 7 wscale_mine 0..14 with
 * window32 0, 1, 65535, 65536 and above; 8 ip_id within 3 of 65535.
 */
#include <arpa/inet.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include REF_TCP_OUT_C

struct mtcp_config CONFIG;

/* ---- stand-ins ------------------------------------------------------------------ */
static unsigned n_timeout_upd, n_arp;
static unsigned char arp_answer[6];
unsigned char *GetDestinationHWaddr(uint32_t dip) { n_arp++; return arp_answer; }
void RequestARP(mtcp_manager_t mtcp, uint32_t ip, int nif, uint32_t cur_ts) { abort(); }
void UpdateTimeoutList(mtcp_manager_t mtcp, tcp_stream *cur_stream) { n_timeout_upd++; }
void AddtoRTOList(mtcp_manager_t mtcp, tcp_stream *cur_stream) { abort(); }   /* payloadlen is 0 */

/* ---- the slot source ------------------------------------------------------------ */
#define MAX_FRAMES 80
static uint8_t slots[MAX_FRAMES][66];
static unsigned slots_used, slot_budget;
static uint8_t *get_wptr(struct mtcp_thread_context *ctx, int ifidx, uint16_t len)
{
    if (len != 66) abort();
    if (slots_used >= slot_budget) return NULL;
    if (slots_used >= MAX_FRAMES) abort();
    memset(slots[slots_used], 0xEE, 66);
    return slots[slots_used++];
}
static io_module_func iom;

/* ---- a small generator (its stream of numbers is not part of any contract) ---- */
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

#define NIFS 3
static mtcp_manager_t mtcp;
static struct tcp_ring_buffer rb;

struct spec {
    uint32_t saddr, daddr, snd_nxt, rcv_nxt, rcv_wnd, head_seq, merged_len, ts_recent, ts_lastack_sent, cur_ts;
    uint16_t sport, dport, ip_id;
    uint8_t ack_cnt, is_wack, wscale_mine, link, has_rcvbuf, need_wnd_adv;
    unsigned budget, n_opts;
    uint8_t opts[128];
};

static void write_state(tcp_stream *st)
{
    w32(st->saddr), w32(st->daddr), w16(st->sport), w16(st->dport);
    w16(st->sndvar->ip_id), w8(st->sndvar->ack_cnt), w8(st->sndvar->is_wack);
    w8(st->sndvar->wscale_mine), w8((uint8_t)st->sndvar->nif_out), w8(st->rcvvar->rcvbuf != NULL), w8(st->need_wnd_adv);
    w32(st->sndvar->ts_lastack_sent), w32(0), w32(0);
    w32(st->snd_nxt), w32(st->rcv_nxt), w32(st->rcvvar->rcv_wnd);
    w32(rb.head_seq), w32((uint32_t)rb.merged_len), w32(st->rcvvar->ts_recent);
}

static struct spec base(void)
{
    struct spec s;
    memset(&s, 0, sizeof(s));
    s.saddr = rnd(), s.daddr = rnd(), s.sport = (uint16_t)rnd(), s.dport = (uint16_t)rnd();
    s.snd_nxt = below(4) ? rnd() : below(3);                      /* 0: the probe's seq wraps */
    s.head_seq = below(4) ? rnd() : 0xFFFFFFFFu - below(2000);
    s.merged_len = below(60000);
    s.rcv_nxt = s.head_seq + s.merged_len;
    s.rcv_wnd = 1 + below(1u << 20);
    s.ts_recent = rnd(), s.ts_lastack_sent = rnd(), s.cur_ts = rnd();
    s.ip_id = (uint16_t)rnd();
    s.wscale_mine = (uint8_t)below(15), s.link = (uint8_t)below(NIFS);
    s.has_rcvbuf = 1;
    s.budget = MAX_FRAMES;
    return s;
}

static void run_case(int fam, const struct spec *s)
{
    tcp_stream st;
    struct tcp_recv_vars rv;
    struct tcp_send_vars sv;
    memset(&st, 0, sizeof(st)), memset(&rv, 0, sizeof(rv)), memset(&sv, 0, sizeof(sv)), memset(&rb, 0, sizeof(rb));
    st.rcvvar = &rv, st.sndvar = &sv;
    st.state = TCP_ST_ESTABLISHED;
    st.on_rto_idx = -1;
    st.saw_timestamp = below(2);                                  /* the options are written either way */
    st.saddr = s->saddr, st.daddr = s->daddr, st.sport = s->sport, st.dport = s->dport;
    st.snd_nxt = s->snd_nxt, st.rcv_nxt = s->rcv_nxt, st.need_wnd_adv = s->need_wnd_adv;
    rv.rcv_wnd = s->rcv_wnd, rv.ts_recent = s->ts_recent;
    rb.head_seq = s->head_seq, rb.merged_len = s->merged_len;
    rv.rcvbuf = s->has_rcvbuf ? &rb : NULL;
    sv.ip_id = s->ip_id, sv.ack_cnt = s->ack_cnt, sv.is_wack = s->is_wack, sv.wscale_mine = s->wscale_mine;
    sv.nif_out = s->link, sv.ts_lastack_sent = s->ts_lastack_sent;
    sv.mss = 1460, sv.eff_mss = 1448;
    struct mtcp_sender *sender = mtcp->n_sender[s->link];
    if (sv.ack_cnt || sv.is_wack) {                               /* it is on the list from before */
        sv.on_ack_list = TRUE;
        TAILQ_INSERT_TAIL(&sender->ack_list, &st, sndvar->ack_link);
        sender->ack_list_cnt++;
    }
    arp_answer[0] = 2, arp_answer[1] = arp_answer[2] = arp_answer[3] = arp_answer[4] = 0, arp_answer[5] = s->link;

    write_state(&st);
    w32(s->cur_ts), w16((uint16_t)s->budget), w16((uint16_t)s->n_opts);
    const long frames_at = ftell(out);
    w16(0), w8((uint8_t)fam), w8(0);
    for (unsigned i = 0; i < ((s->n_opts + 3) & ~3u); ++i) w8(i < s->n_opts ? s->opts[i] : 0xFF);

    for (unsigned i = 0; i < s->n_opts; ++i) EnqueueACK(mtcp, &st, s->cur_ts, s->opts[i]);
    slots_used = 0, slot_budget = s->budget, n_timeout_upd = 0;
    const uint32_t snd_nxt = st.snd_nxt, last_active = st.last_active_ts;
    const int listed = sv.on_ack_list;
    if (sender->ack_list_cnt != (listed ? 1 : 0)) abort();
    WriteTCPACKList(mtcp, sender, s->cur_ts, 1 << 20);
    /* what the tx record calls fixed, and what a pure ACK must not touch */
    if (st.saddr != s->saddr || st.daddr != s->daddr || st.sport != s->sport || st.dport != s->dport ||
        sv.wscale_mine != s->wscale_mine || sv.nif_out != s->link || (rv.rcvbuf != NULL) != s->has_rcvbuf ||
        st.snd_nxt != snd_nxt || st.rcv_nxt != s->rcv_nxt || rv.rcv_wnd != s->rcv_wnd ||
        rv.ts_recent != s->ts_recent || rb.head_seq != s->head_seq || rb.merged_len != s->merged_len ||
        st.on_rto_idx != -1 || sv.ts_rto != 0 || sv.on_send_list || sv.on_control_list)
        abort();
    if (n_timeout_upd != slots_used) abort();                     /* tcp_out.c:292, once per frame */
    if (slots_used && st.last_active_ts != s->cur_ts) abort();    /* tcp_out.c:291 */
    if (!slots_used && st.last_active_ts != last_active) abort();
    if (sender->ack_list_cnt != (sv.on_ack_list ? 1 : 0)) abort();
    if (sv.on_ack_list) {                                         /* take it off for the next case */
        TAILQ_REMOVE(&sender->ack_list, &st, sndvar->ack_link);
        sender->ack_list_cnt--;
    }
    fwrite(slots, 66, slots_used, out);
    write_state(&st);
    const long end = ftell(out);
    fseek(out, frames_at, SEEK_SET);
    w16((uint16_t)slots_used), w8((uint8_t)fam), w8(sv.on_ack_list);
    fseek(out, end, SEEK_SET);
    n_cases++;
}

static void opts_fill(struct spec *s, unsigned n, int kind)
{
    s->n_opts = n;
    for (unsigned i = 0; i < n; ++i) s->opts[i] = kind == 2 ? (uint8_t)below(2) : (uint8_t)kind;
}

int main(int argc, char **argv)
{
    if (argc < 2 || !(out = fopen(argv[1], "wb"))) return 2;
    mtcp = calloc(1, sizeof(*mtcp));
    iom.get_wptr = get_wptr;
    mtcp->iom = &iom;
    CONFIG.eths_num = NIFS;
    CONFIG.eths = calloc(NIFS, sizeof(*CONFIG.eths));
    CONFIG.nif_to_eidx = calloc(NIFS, sizeof(int));
    for (int i = 0; i < NIFS; ++i) {
        CONFIG.nif_to_eidx[i] = i;
        CONFIG.eths[i].haddr[0] = 2, CONFIG.eths[i].haddr[1] = 1, CONFIG.eths[i].haddr[5] = (unsigned char)i;
        mtcp->n_sender[i] = calloc(1, sizeof(struct mtcp_sender));
        TAILQ_INIT(&mtcp->n_sender[i]->ack_list);
        TAILQ_INIT(&mtcp->n_sender[i]->send_list);
        TAILQ_INIT(&mtcp->n_sender[i]->control_list);
    }
    w32(0x474B4341u), w32(1), w32(0), w32(0);                     /* 'ACKG' */

    struct spec s;
    for (unsigned k = 1; k <= 6; ++k) {                           /* 0: AGGREGATE only */
        s = base(), opts_fill(&s, k, ACK_OPT_AGGREGATE), run_case(0, &s);
    }
    for (unsigned k = 1; k <= 70; ++k) {                          /* 1: k NOWs */
        s = base(), opts_fill(&s, k, ACK_OPT_NOW), run_case(1, &s);
    }
    for (unsigned i = 0; i < 120; ++i) {                          /* 2: mixed, a count on entry */
        s = base(), s.ack_cnt = (uint8_t)(1 + (i < 40 ? 58 + below(5) : below(63)));
        opts_fill(&s, 1 + below(i < 40 ? 12 : 100), 2), run_case(2, &s);
    }
    for (unsigned i = 0; i < 40; ++i) {                           /* 3: is_wack */
        s = base(), s.is_wack = 1;
        if (i & 1) opts_fill(&s, 1 + below(5), 2);
        if (i % 4 == 2) s.n_opts = 1, s.opts[0] = ACK_OPT_WACK, s.is_wack = 0;
        run_case(3, &s);
    }
    for (unsigned i = 0; i < 20; ++i) {                           /* 4: rcvbuf == NULL */
        s = base(), s.has_rcvbuf = 0, s.is_wack = (uint8_t)(i & 1), opts_fill(&s, 1 + below(9), 2), run_case(4, &s);
    }
    for (unsigned i = 0; i < 30; ++i) {                           /* 5: rcv_nxt against head_seq + merged_len */
        s = base();
        const uint32_t d[6] = {1, 2, 1000, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
        s.rcv_nxt = s.head_seq + s.merged_len + d[i % 6];
        s.is_wack = (uint8_t)(i & 1), opts_fill(&s, 1 + below(9), 2), run_case(5, &s);
    }
    for (unsigned i = 0; i < 60; ++i) {                           /* 6: the slot budget */
        s = base();
        const unsigned k = 2 + below(20);
        opts_fill(&s, k, ACK_OPT_NOW), s.is_wack = 1;
        s.budget = i % 3 == 0 ? 0 : i % 3 == 1 ? k : 1 + below(k - 1);
        if (i >= 45) s.is_wack = 0, s.budget = below(k);
        run_case(6, &s);
    }
    for (unsigned ws = 0; ws <= 14; ++ws) {                       /* 7: the window */
        const uint64_t w32s[7] = {0, 1, 65534, 65535, 65536, 65537, 100000};
        for (unsigned j = 0; j < 7; ++j) {
            const uint64_t wnd = (w32s[j] << ws) + (ws ? below(1u << ws) : 0);
            if (wnd > 0xFFFFFFFFull) continue;
            s = base(), s.wscale_mine = (uint8_t)ws, s.rcv_wnd = (uint32_t)wnd, s.need_wnd_adv = (uint8_t)below(2);
            s.is_wack = (uint8_t)(j & 1), opts_fill(&s, 1 + below(3), 2), run_case(7, &s);
        }
    }
    for (unsigned i = 0; i < 14; ++i) {                           /* 8: ip_id near the wrap */
        s = base(), s.ip_id = (uint16_t)(65535 - 3 + i % 7), s.is_wack = (uint8_t)(i & 1);
        opts_fill(&s, 1 + below(8), ACK_OPT_NOW), run_case(8, &s);
    }
    fseek(out, 8, SEEK_SET);
    w32(n_cases);
    fclose(out);
    printf("%u cases\n", n_cases);
    return 0;
}
