/*
 * ref_datagen_gen.c — TEST INFRASTRUCTURE ONLY: writes tests/golden/datagen_cases.bin
 * with the reference's own data sending (tests/make_datagen_golden.py compiles and
 * runs it where the reference's sources are present; nothing of them is copied:
 * tcp_out.c comes in by path, which makes its static FlushTCPSendingBuffer and
 * GenerateTCPOptions and its inline WriteTCPDataList, SendTCPPacket, EnqueueACK and
 * AddtoSendList reachable).
 *
 * Which output path runs: the reference's own IPOutput (ip_out.c, linked) and
 * its own EthernetOutput (eth_out.c, linked), with stand-ins in this file for
 * GetDestinationHWaddr and RequestARP, against this file's slot source: an
 * io_module whose get_wptr hands out slots and runs dry after `budget` of
 * them.  tcp_util.c is linked for TCPCalcChecksum, timer.c for the reference's
 * own AddtoRTOList (whose guard is timer.c:37) on a real RTO store and its own
 * UpdateTimeoutList.
 *
 * Per case the driver fills 1 to 8 streams, puts those with on_send_list on the
 * sender's send list in order and calls WriteTCPDataList once.  In a list only
 * the last stream may end with ret < 0, so every listed stream is served in
 * that one call (tcp_out.c:633-636 breaks at the first negative ret).  ret is
 * recovered from what the call leaves: on_send_list cleared means ret >= 0 and
 * ret = the frames written; else -1 with on_control_list, -2 where the slots
 * ran dry, -3 otherwise.  The driver aborts if a field the records call fixed
 * has changed, or if last_active_ts was not set where a frame went out.
 * on_ack_list is FALSE on entry whatever is_wack says, so that it tells after
 * the call whether EnqueueACK(ACK_OPT_WACK) ran (tcp_out.c:429-431).
 *
 * The file: u32 magic 'DGEN', u32 version, u32 cases, u32 0; per case
 *   u32 cur_ts; u16 the slot budget; u8 family; u8 streams;
 *   per stream, before: a stream record, then u32 the send buffer's bytes, then
 *     those bytes (from the byte with sequence number head_seq), padded to 4;
 *   per stream, after: i32 ret (0x7FFFFFFF: not on the list, not served);
 *     u16 frames; u8 1 if the RTO list took the stream in; u8 on_ack_list;
 *     a stream record; per frame u16 length, u16 0, the frame padded to 4.
 * A stream record, 88 B: the 32 B of struct mtcp_gpu_ackgen_state
 * (include/mtcp_gpu_ackgen.h); u32 snd_nxt, snd_una, peer_wnd, cwnd, rto, ts_rto,
 * sndbuf head_seq, sndbuf len; u16 mss; u8 on_rto, has_sndbuf, on_send_list,
 * on_control_list; u16 0; u32 rcv_nxt, rcv_wnd, ts_recent; u32 the offset the
 * tests give the buffer's first byte in their payload arena.  link is
 * sndvar->nif_out, the Ethernet addresses being 02:00:00:00:00:<link> (the ARP
 * answer) and 02:01:00:00:00:<link> (CONFIG.eths[].haddr).  All little-endian.
 *
 * Families: 0 a buffer that fits the window, lengths around multiples of
 * mss - 12, mss 13, 14, 64, 536, 1460; 1 the cwnd stop and the peer-window stop
 * on the first segment and after some; 2 the 500 ms test at 499, 500, 501 and
 * where the difference times 1000 wraps 32 bits; 3 snd_nxt in mid-buffer, at
 * the buffer's end and behind head_seq; 4 the state right after a fast
 * retransmit; 5 sb_len 0, no send buffer, on_control_list; 6 slot budgets that
 * cut at 0, inside and before the last segment; 7 ack_cnt 0, 1, equal to ret,
 * above ret and 63, with ret >= 0 and ret < 0; 8 seq and ip_id across their
 * wraps; 9 a zero advertised window; 10 not on the send list; 11 lists of 2-8
 * streams where only the last may stall.  on_rto is 0 or 1 and the arena
 * offsets are odd throughout.
 */
#include <arpa/inet.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include REF_TCP_OUT_C

#include "timer.h"

struct mtcp_config CONFIG;

/* ---- stand-ins ------------------------------------------------------------------ */
static unsigned char arp_answer[6];
unsigned char *GetDestinationHWaddr(uint32_t dip) { return arp_answer; }
void RequestARP(mtcp_manager_t mtcp, uint32_t ip, int nif, uint32_t cur_ts) { abort(); }

/* ---- the slot source ------------------------------------------------------------ */
#define MAX_FRAMES 96
#define SLOT 1600
static uint8_t slots[MAX_FRAMES][SLOT];
static uint16_t slot_len[MAX_FRAMES];
static unsigned slots_used, slot_budget;
static uint8_t *get_wptr(struct mtcp_thread_context *ctx, int ifidx, uint16_t len)
{
    if (len > SLOT || len < 67) abort();
    if (slots_used >= slot_budget) return NULL;
    if (slots_used >= MAX_FRAMES) abort();
    memset(slots[slots_used], 0xEE, SLOT);
    slot_len[slots_used] = len;
    return slots[slots_used++];
}
static io_module_func iom;

/* ---- a small generator (its stream of numbers is not part of any contract) ---- */
static uint64_t rng_s = 0xA0761D6478BD642Full;
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
static void wpad(const uint8_t *p, unsigned n)
{
    static const uint8_t z[4];
    fwrite(p, 1, n, out);
    fwrite(z, 1, (4 - (n & 3)) & 3, out);
}

#define NIFS 3
#define MAX_STREAMS 8
#define SB_MAX 8192
static mtcp_manager_t mtcp;

struct spec {
    uint32_t saddr, daddr, ts_lastack_sent;
    uint16_t sport, dport, ip_id, mss;
    uint8_t ack_cnt, is_wack, wscale_mine, link, need_wnd_adv;
    uint32_t snd_nxt, snd_una, peer_wnd, cwnd, rto, ts_rto, head_seq, sb_len;
    uint8_t on_rto, has_sndbuf, on_send_list, on_control_list;
    uint32_t rcv_nxt, rcv_wnd, ts_recent, arena_off;
};

struct live {
    tcp_stream st;
    struct tcp_recv_vars rv;
    struct tcp_send_vars sv;
    struct tcp_send_buffer sb;
    struct tcp_ring_buffer rb;
    uint8_t bytes[SB_MAX];
};
static struct live lv[MAX_STREAMS];

static void write_record(const struct live *k, uint32_t arena_off)
{
    const tcp_stream *st = &k->st;
    w32(st->saddr), w32(st->daddr), w16(st->sport), w16(st->dport);
    w16(k->sv.ip_id), w8(k->sv.ack_cnt), w8(k->sv.is_wack);
    w8(k->sv.wscale_mine), w8((uint8_t)k->sv.nif_out), w8(k->rv.rcvbuf != NULL), w8(st->need_wnd_adv);
    w32(k->sv.ts_lastack_sent), w32(0), w32(0);
    w32(st->snd_nxt), w32(k->sv.snd_una), w32(k->sv.peer_wnd), w32(k->sv.cwnd);
    w32(k->sv.rto), w32(k->sv.ts_rto), w32(k->sb.head_seq), w32(k->sb.len);
    w16(k->sv.mss), w8(st->on_rto_idx >= 0), w8(k->sv.sndbuf != NULL), w8(k->sv.on_send_list), w8(k->sv.on_control_list);
    w16(0);
    w32(st->rcv_nxt), w32(k->rv.rcv_wnd), w32(k->rv.ts_recent), w32(arena_off);
}

/* a stream with an open window and a buffer of `len` bytes, snd_nxt at its head */
static struct spec base(uint16_t mss, uint32_t len)
{
    struct spec s;
    memset(&s, 0, sizeof(s));
    s.saddr = rnd(), s.daddr = rnd(), s.sport = (uint16_t)rnd(), s.dport = (uint16_t)rnd();
    s.ip_id = (uint16_t)rnd(), s.mss = mss;
    s.wscale_mine = (uint8_t)below(15), s.link = (uint8_t)below(NIFS);
    s.ts_lastack_sent = rnd();
    s.head_seq = rnd(), s.sb_len = len;
    s.snd_una = s.head_seq, s.snd_nxt = s.head_seq;
    s.peer_wnd = len + 1 + below(100000), s.cwnd = len + 1 + below(100000);
    s.rto = 1 + below(3000), s.ts_rto = rnd();
    s.on_rto = (uint8_t)below(2), s.has_sndbuf = 1, s.on_send_list = 1;
    s.rcv_nxt = rnd(), s.rcv_wnd = (1u << s.wscale_mine) + below(1u << 20), s.ts_recent = rnd();
    return s;
}

static void run_case(int fam, struct spec *sp, unsigned n, uint32_t cur_ts, unsigned budget)
{
    if (n < 1 || n > MAX_STREAMS) abort();
    struct mtcp_sender *sender = mtcp->n_sender[sp[0].link];
    uint32_t arena = 1;
    arp_answer[5] = sp[0].link;
    w32(cur_ts), w16((uint16_t)budget), w8((uint8_t)fam), w8((uint8_t)n);
    for (unsigned i = 0; i < n; ++i) {
        struct spec *s = &sp[i];
        struct live *k = &lv[i];
        if (s->sb_len > SB_MAX || s->link != sp[0].link) abort();
        /* timer.c:47-49 indexes its store by ts_rto - rto_now_ts, which must not be negative: a stream on
         * the RTO list from before has ts_rto = cur_ts, and a list's rto values ascend */
        if (s->on_rto) s->ts_rto = cur_ts;
        if (i && s->rto < sp[i - 1].rto) abort();
        memset(&k->st, 0, sizeof(k->st)), memset(&k->rv, 0, sizeof(k->rv)), memset(&k->sv, 0, sizeof(k->sv));
        memset(&k->sb, 0, sizeof(k->sb)), memset(&k->rb, 0, sizeof(k->rb));
        tcp_stream *st = &k->st;
        st->rcvvar = &k->rv, st->sndvar = &k->sv;
        st->state = TCP_ST_ESTABLISHED;
        st->on_rto_idx = -1;
        st->saw_timestamp = below(2);                             /* the options are written either way */
        st->saddr = s->saddr, st->daddr = s->daddr;
        st->sport = s->sport, st->dport = s->dport;
        st->snd_nxt = s->snd_nxt, st->rcv_nxt = s->rcv_nxt, st->need_wnd_adv = s->need_wnd_adv;
        k->rv.rcv_wnd = s->rcv_wnd, k->rv.ts_recent = s->ts_recent, k->rv.rcvbuf = &k->rb;
        k->sv.ip_id = s->ip_id, k->sv.ack_cnt = s->ack_cnt, k->sv.is_wack = s->is_wack;
        k->sv.wscale_mine = s->wscale_mine, k->sv.nif_out = s->link, k->sv.ts_lastack_sent = s->ts_lastack_sent;
        k->sv.mss = s->mss, k->sv.eff_mss = s->mss - 12;
        k->sv.snd_una = s->snd_una, k->sv.peer_wnd = s->peer_wnd, k->sv.cwnd = s->cwnd;
        k->sv.rto = s->rto, k->sv.ts_rto = s->ts_rto;
        for (uint32_t b = 0; b < s->sb_len; ++b) k->bytes[b] = (uint8_t)rnd();
        k->sb.data = k->sb.head = k->bytes, k->sb.len = s->sb_len, k->sb.size = SB_MAX, k->sb.head_seq = s->head_seq;
        k->sv.sndbuf = s->has_sndbuf ? &k->sb : NULL;
        k->sv.on_control_list = s->on_control_list;
        SBUF_LOCK_INIT(&k->sv.write_lock, "write_lock", abort());    /* tcp_out.c:375 takes it */
        if (s->on_rto) {                                          /* it is on the RTO list from before */
            AddtoRTOList(mtcp, st);
            if (st->on_rto_idx < 0) abort();
        }
        if (s->on_send_list) {                                    /* tcp_out.c:850-851 */
            k->sv.on_send_list = TRUE;
            TAILQ_INSERT_TAIL(&sender->send_list, st, sndvar->send_link);
            sender->send_list_cnt++;
        }
        s->arena_off = arena + 2 * below(40);                     /* odd, streams apart */
        arena = s->arena_off + s->sb_len + (s->sb_len & 1) + 2;
        write_record(k, s->arena_off);
        w32(s->has_sndbuf ? s->sb_len : 0);
        if (s->has_sndbuf) wpad(k->bytes, s->sb_len);
    }
    slots_used = 0, slot_budget = budget;
    WriteTCPDataList(mtcp, sender, cur_ts, 1 << 20);
    unsigned frame = 0;
    for (unsigned i = 0; i < n; ++i) {
        const struct spec *s = &sp[i];
        struct live *k = &lv[i];
        tcp_stream *st = &k->st;
        /* the frames of this stream: those whose ports and addresses are its own, in slot order */
        unsigned first = frame;
        const uint32_t sent = st->snd_nxt - s->snd_nxt;
        uint32_t got = 0;
        while (got < sent) {
            if (frame >= slots_used) abort();
            got += slot_len[frame] - 66u;
            frame++;
        }
        if (got != sent) abort();
        const unsigned nf = frame - first;
        int ret;
        if (!s->on_send_list) ret = 0x7FFFFFFF;
        else if (!k->sv.on_send_list) ret = (int)nf;              /* tcp_out.c:639 ran: ret >= 0, the packets sent */
        else if (s->on_control_list) ret = -1;                    /* tcp_out.c:617 */
        else if (slots_used >= slot_budget && i == n - 1) ret = -2;    /* tcp_out.c:238-240, :439-441 */
        else ret = -3;                                            /* tcp_out.c:433 */
        if (ret < 0 && i != n - 1) abort();                       /* only the last may stall */
        /* what the records call fixed, and what the call must not touch */
        if (st->saddr != s->saddr || st->daddr != s->daddr || st->sport != s->sport || st->dport != s->dport ||
            k->sv.wscale_mine != s->wscale_mine || k->sv.nif_out != s->link || st->rcv_nxt != s->rcv_nxt ||
            k->rv.rcv_wnd != s->rcv_wnd || k->rv.ts_recent != s->ts_recent || k->sv.snd_una != s->snd_una ||
            k->sv.peer_wnd != s->peer_wnd || k->sv.cwnd != s->cwnd || k->sv.rto != s->rto ||
            k->sb.head_seq != s->head_seq || k->sb.len != s->sb_len || k->sv.mss != s->mss ||
            k->sv.on_control_list != s->on_control_list || (k->sv.sndbuf != NULL) != s->has_sndbuf)
            abort();
        if (nf && st->last_active_ts != cur_ts) abort();          /* tcp_out.c:291 */
        w32((uint32_t)ret), w16((uint16_t)nf), w8(st->on_rto_idx >= 0 && !s->on_rto), w8(k->sv.on_ack_list);
        write_record(k, s->arena_off);
        for (unsigned f = first; f < frame; ++f) w16(slot_len[f]), w16(0), wpad(slots[f], slot_len[f]);
        /* take it off every list for the next case */
        if (k->sv.on_send_list) {
            TAILQ_REMOVE(&sender->send_list, st, sndvar->send_link);
            sender->send_list_cnt--;
        }
        if (k->sv.on_ack_list) {
            TAILQ_REMOVE(&sender->ack_list, st, sndvar->ack_link);
            sender->ack_list_cnt--;
        }
        if (st->on_rto_idx >= 0) RemoveFromRTOList(mtcp, st);
    }
    if (frame != slots_used || sender->send_list_cnt || sender->ack_list_cnt || mtcp->rto_list_cnt) abort();
    n_cases++;
}

static void one(int fam, struct spec s, uint32_t cur_ts, unsigned budget) { run_case(fam, &s, 1, cur_ts, budget); }

int main(int argc, char **argv)
{
    if (argc < 2 || !(out = fopen(argv[1], "wb"))) return 2;
    mtcp = calloc(1, sizeof(*mtcp));
    iom.get_wptr = get_wptr;
    mtcp->iom = &iom;
    mtcp->rto_store = InitRTOHashstore();
    if (!mtcp->rto_store) abort();
    CONFIG.eths_num = NIFS;
    CONFIG.eths = calloc(NIFS, sizeof(*CONFIG.eths));
    CONFIG.nif_to_eidx = calloc(NIFS, sizeof(int));
    arp_answer[0] = 2;
    for (int i = 0; i < NIFS; ++i) {
        CONFIG.nif_to_eidx[i] = i;
        CONFIG.eths[i].haddr[0] = 2, CONFIG.eths[i].haddr[1] = 1, CONFIG.eths[i].haddr[5] = (unsigned char)i;
        mtcp->n_sender[i] = calloc(1, sizeof(struct mtcp_sender));
        TAILQ_INIT(&mtcp->n_sender[i]->ack_list);
        TAILQ_INIT(&mtcp->n_sender[i]->send_list);
        TAILQ_INIT(&mtcp->n_sender[i]->control_list);
    }
    w32(0x4E454744u), w32(1), w32(0), w32(0);                     /* 'DGEN' */

    static const uint16_t MSS[5] = {13, 14, 64, 536, 1460};
    struct spec s;
    for (unsigned mi = 0; mi < 5; ++mi) {                         /* 0: fits the window */
        const uint32_t m = MSS[mi] - 12u;
        const unsigned kmax = MSS[mi] >= 536 ? 2 : 5;
        for (unsigned k = 0; k <= kmax; ++k) {
            const uint32_t tails[3] = {0, 1, m - 1};
            for (unsigned t = 0; t < 3; ++t) {
                const uint32_t len = k * m + tails[t];
                if (len == 0 || len > SB_MAX || (m == 1 && t)) continue;
                s = base(MSS[mi], len), one(0, s, rnd(), MAX_FRAMES);
            }
        }
    }
    for (unsigned i = 0; i < 48; ++i) {                           /* 1: the window stops */
        const uint16_t mss = MSS[1 + i % 3];
        const uint32_t m = mss - 12u, segs = 4, len = segs * m + below(m);
        s = base(mss, len);
        const uint32_t infl = below(3) ? below(500) : 0;
        s.snd_una = s.head_seq - infl;                            /* bytes in flight in front of the buffer's head */
        const uint32_t after = (i / 3) % 4;                       /* full segments that pass */
        const uint32_t wnd = infl + after * m + (after ? below(m) : (below(2) ? below(m) : 0));
        if (i % 2) s.cwnd = wnd, s.peer_wnd = wnd + 1 + below(5000);      /* cwnd stops it: peer_wnd may or may not */
        else s.peer_wnd = wnd, s.cwnd = wnd + below(5000);
        if (i % 8 == 7) s.cwnd = wnd, s.peer_wnd = infl + len + 10;       /* the peer window is open: no probe */
        s.ts_lastack_sent = 0;
        one(1, s, 100000 + below(1000), MAX_FRAMES);
    }
    {                                                             /* 2: the 500 ms test */
        const uint32_t d[9] = {0, 499, 500, 501, 4294968u, 4295468u, 4295469u, 0x80000000u, 0xFFFFFFFFu};
        for (unsigned i = 0; i < 18; ++i) {
            s = base(64, 200);
            s.peer_wnd = i & 1 ? 60 : 10, s.cwnd = s.peer_wnd + below(3);    /* with and without segments in front */
            const uint32_t cur_ts = rnd();
            s.ts_lastack_sent = cur_ts - d[i / 2];
            s.is_wack = (uint8_t)(i % 3 == 0);
            one(2, s, cur_ts, MAX_FRAMES);
        }
    }
    for (unsigned i = 0; i < 24; ++i) {                           /* 3: where snd_nxt is */
        const uint16_t mss = MSS[i % 4];
        const uint32_t m = mss - 12u, len = 3 * m + below(m);
        s = base(mss, len);
        s.snd_una = s.head_seq;
        if (i % 3 == 0) s.snd_nxt = s.head_seq + 1 + below(len - 1);         /* mid-buffer */
        else if (i % 3 == 1) s.snd_nxt = s.head_seq + len;                   /* at its end: nothing to send */
        else s.snd_nxt = s.head_seq - 1 - below(1000), s.snd_una = s.snd_nxt;   /* behind head_seq */
        s.peer_wnd += 2000, s.cwnd += 2000;
        s.ack_cnt = (uint8_t)below(4);
        one(3, s, rnd(), MAX_FRAMES);
    }
    for (unsigned i = 0; i < 16; ++i) {                           /* 4: right after a fast retransmit (tcp_in.c:392-426) */
        const uint16_t mss = MSS[1 + i % 3];
        const uint32_t m = mss - 12u, len = 6 * m + below(m);
        s = base(mss, len);
        s.snd_una = s.snd_nxt = s.head_seq;                       /* tcp_in.c:406: snd_nxt = ack_seq */
        const uint32_t ssthresh = 2 * mss + below(2 * mss);       /* tcp_in.c:411-415 */
        s.cwnd = ssthresh + 3 * mss;                              /* tcp_in.c:418 */
        s.peer_wnd = below(2) ? s.cwnd + below(4000) : below(s.cwnd + 1);
        s.on_rto = 1;
        one(4, s, rnd(), MAX_FRAMES);
    }
    for (unsigned i = 0; i < 12; ++i) {                           /* 5: nothing to flush */
        s = base(MSS[i % 5], 100);
        if (i % 3 == 0) s.sb_len = 0, s.snd_nxt = s.head_seq;
        else if (i % 3 == 1) s.has_sndbuf = 0;
        else s.on_control_list = 1;
        s.ack_cnt = (uint8_t)below(5);
        one(5, s, rnd(), MAX_FRAMES);
    }
    for (unsigned i = 0; i < 30; ++i) {                           /* 6: the slot budget */
        const uint16_t mss = MSS[i % 3];
        const uint32_t m = mss - 12u, segs = 2 + below(10), len = (segs - 1) * m + 1 + below(m);
        s = base(mss, len);
        const unsigned budget = i % 3 == 0 ? 0 : i % 3 == 1 ? segs - 1 : below(segs);
        s.ack_cnt = (uint8_t)below(6);
        one(6, s, rnd(), budget);
    }
    for (unsigned i = 0; i < 40; ++i) {                           /* 7: the piggy-back decrement */
        const uint16_t mss = MSS[i % 3];
        const uint32_t m = mss - 12u, segs = 1 + below(6), len = segs * m;
        s = base(mss, len);
        const uint8_t cnts[5] = {0, 1, (uint8_t)segs, (uint8_t)(segs + 1 + below(5)), 63};
        s.ack_cnt = cnts[i % 5];
        if ((i / 5) % 2) s.cwnd = s.peer_wnd = (segs - 1) * m + below(m);    /* ret -3 behind segs - 1 segments */
        one(7, s, rnd(), MAX_FRAMES);
    }
    for (unsigned i = 0; i < 16; ++i) {                           /* 8: the wraps */
        const uint16_t mss = MSS[1 + i % 2];
        const uint32_t m = mss - 12u, len = 5 * m + below(m);
        s = base(mss, len);
        s.ip_id = (uint16_t)(65535 - below(5));
        s.head_seq = 0xFFFFFFFFu - below(3 * m), s.snd_una = s.head_seq - below(50);
        s.snd_nxt = s.head_seq + (i & 1 ? below(m) : 0);
        s.peer_wnd += 200, s.cwnd += 200;
        one(8, s, i & 2 ? 0xFFFFFFFFu - below(100) : rnd(), MAX_FRAMES);
    }
    for (unsigned i = 0; i < 12; ++i) {                           /* 9: a zero advertised window */
        s = base(MSS[i % 3], 30 + below(40));
        s.wscale_mine = (uint8_t)(1 + below(14));
        s.rcv_wnd = i % 3 == 2 ? 1u << s.wscale_mine : below(1u << s.wscale_mine);
        s.need_wnd_adv = (uint8_t)(i & 1);
        if (i % 4 == 3) s.cwnd = s.peer_wnd = 0;                  /* nothing goes out: need_wnd_adv stays */
        one(9, s, rnd(), MAX_FRAMES);
    }
    for (unsigned i = 0; i < 4; ++i) {                            /* 10: not on the send list */
        s = base(MSS[i % 3], 50), s.on_send_list = 0, s.ack_cnt = 3;
        one(10, s, rnd(), MAX_FRAMES);
    }
    for (unsigned i = 0; i < 28; ++i) {                           /* 11: lists */
        struct spec l[MAX_STREAMS];
        const unsigned n = 2 + i % 7;
        const uint8_t link = (uint8_t)below(NIFS);
        unsigned frames = 0;
        for (unsigned j = 0; j < n; ++j) {
            const uint16_t mss = MSS[below(3)];
            const uint32_t m = mss - 12u, segs = below(5);
            l[j] = base(mss, segs * m + below(m));
            l[j].link = link;
            l[j].rto = 400 * j + 1 + below(400);
            l[j].ack_cnt = (uint8_t)below(4);
            if (l[j].sb_len == 0) l[j].sb_len = 1;
            if (below(5) == 0) l[j].on_send_list = 0;
            if (below(6) == 0) l[j].snd_nxt = l[j].head_seq + l[j].sb_len;   /* nothing to send */
        }
        unsigned budget = MAX_FRAMES;
        struct spec *last = &l[n - 1];
        last->on_send_list = 1;
        for (unsigned j = 0; j < n; ++j) {
            const uint32_t m = l[j].mss - 12u;
            if (l[j].on_send_list) frames += (l[j].head_seq + l[j].sb_len - l[j].snd_nxt + m - 1) / m;
        }
        if (i % 4 == 1) last->cwnd = below(last->sb_len + 1);                /* -3 */
        else if (i % 4 == 2) last->on_control_list = 1;                      /* -1 */
        else if (i % 4 == 3 && last->snd_nxt == last->head_seq && last->sb_len > (uint32_t)last->mss - 12)
            budget = frames - 1;                                             /* -2 inside the last stream */
        run_case(11, l, n, rnd(), budget);
    }
    fseek(out, 8, SEEK_SET);
    w32(n_cases);
    fclose(out);
    printf("%u cases\n", n_cases);
    return 0;
}
