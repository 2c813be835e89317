/*
 * ref_ackwalk_gen.c — TEST INFRASTRUCTURE ONLY: writes tests/golden/ackwalk_cases.bin
 * with the reference's own ACK handling (tests/make_ackwalk_golden.py compiles
 * and runs it where the reference's sources are present; nothing of them is
 * copied: tcp_in.c comes in by path, which makes its static inline
 * ValidateSequence, Handle_TCP_ST_ESTABLISHED and through it ProcessACK
 * reachable; tcp_send_buffer.c (SBRemove), timer.c (UpdateRetransmissionTimer
 * and the RTO list it keeps), tcp_util.c, tcp_ring_buffer.c, memory_mgt.c,
 * tcp_rb_frag_queue.c and tcp_sb_queue.c are linked).
 *
 * Per packet the driver does what ProcessTCPPacket does behind StreamHTSearch
 * for an ESTABLISHED stream (mtcp/src/tcp_in.c:1194-1209, :1256-1258):
 * ValidateSequence, and Handle_TCP_ST_ESTABLISHED if it returned TRUE, on a
 * stream with a real receive buffer and a real send buffer: the receive steps
 * and the ACK steps run interleaved, as in the reference.  RaiseWriteEvent,
 * AddtoSendList, RemoveFromSendList, EnqueueACK and RaiseReadEvent are this
 * file's: they count the calls.  timer.c's own AddtoRTOList and
 * RemoveFromRTOList run on a real RTO store (UpdateRetransmissionTimer calls
 * them inside its own translation unit); their calls are read off
 * on_rto_idx and rto_list_cnt around the packet.
 *
 * Each packet is made from the stream's state at that point, so that the
 * walks reach what they aim at; the inputs stay inside the range where the
 * reference has no undefined behaviour (mss * packets and packets * mss * mss
 * inside int, cwnd and eff_mss not 0, wscale at most 7, an ACK at most the send
 * buffer's length ahead or 3 000 behind).  The driver aborts
 * if a packet changes a field the state record calls fixed.
 *
 * The file: u32 magic 'ACKW', u32 version, u32 walks, u32 packets per walk;
 * per walk the 88 B of the send state before the first packet (the layout of
 * struct mtcp_gpu_ack_state, include/mtcp_gpu_ackwalk.h), u32 family, u32
 * packets; per packet
 *   in:  u32 seq, ack_seq, ts_ref, cur_ts; u16 window, payload_len; u8 the ACK
 *        flag, u8 the packet carries NOP NOP TS, i8 ValidateSequence's return,
 *        u8 0;
 *   out: u8 RaiseWriteEvent calls before SBRemove, after SBRemove,
 *        AddtoSendList, RemoveFromSendList, RemoveFromRTOList, AddtoRTOList
 *        calls, u16 0; u32 the bytes that left the send buffer; the 18 words
 *        at offsets 0-71 of the state record; u8 dup_acks, nrtx, on_rto, 0.
 * All little-endian.
 */
#include <arpa/inet.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include REF_TCP_IN_C

struct mtcp_config CONFIG;

static unsigned n_wev_wnd, n_wev_room, n_add_send, n_rm_send, n_ack, n_read;
static uint32_t sb_len_at_entry;

void EnqueueACK(mtcp_manager_t mtcp, tcp_stream *cur_stream, uint32_t cur_ts, uint8_t opt) { n_ack++; }
void RaiseReadEvent(mtcp_manager_t mtcp, tcp_stream *stream) { n_read++; }
void RaiseWriteEvent(mtcp_manager_t mtcp, tcp_stream *stream)
{
    /* tcp_in.c:362 runs before SBRemove at :511, tcp_in.c:521 behind it */
    if (stream->sndvar->sndbuf->len == sb_len_at_entry) n_wev_wnd++;
    else n_wev_room++;
}
void AddtoSendList(mtcp_manager_t mtcp, tcp_stream *cur_stream) { n_add_send++; }
void RemoveFromSendList(mtcp_manager_t mtcp, tcp_stream *cur_stream) { n_rm_send++; }

/* ---- a small generator (its stream of numbers is not part of any contract) ---- */
static uint64_t rng_s = 0xD1B54A32D192ED03ull;
static uint32_t rnd(void)
{
    rng_s ^= rng_s << 13, rng_s ^= rng_s >> 7, rng_s ^= rng_s << 17;
    return (uint32_t)(rng_s >> 16);
}
static uint32_t below(uint32_t n) { return rnd() % n; }

#define PKTS 16
#define SB_SIZE 65536
#define RB_SIZE 65536

static FILE *out;
static void w32(uint32_t v) { fwrite(&v, 4, 1, out); }
static void w16(uint16_t v) { fwrite(&v, 2, 1, out); }
static void w8(uint8_t v) { fwrite(&v, 1, 1, out); }

static uint8_t payload[65536];

struct walk {
    mtcp_manager_t mtcp;
    tcp_stream st;
    struct tcp_recv_vars rv;
    struct tcp_send_vars sv;
    struct tcp_send_buffer *sb;          /* kept when sv.sndbuf is NULL */
};

static void write_words(struct walk *k)
{
    tcp_stream *st = &k->st;
    w32(st->snd_nxt), w32(k->sv.snd_una), w32(k->sv.snd_wnd), w32(k->sv.peer_wnd);
    w32(k->rv.snd_wl1), w32(k->rv.snd_wl2), w32(k->rv.last_ack_seq), w32(k->sv.cwnd);
    w32(k->sv.ssthresh), w32(k->sv.rto), w32(k->sv.ts_rto), w32(k->rv.srtt);
    w32(k->rv.mdev), w32(k->rv.mdev_max), w32(k->rv.rttvar), w32(k->rv.rtt_seq);
    w32(k->sb->head_seq), w32((uint32_t)k->sb->len);
}

struct fixed {
    uint32_t sb_size;
    uint16_t mss, eff_mss;
    uint8_t state, saw_ts, wscale, has_sndbuf;
};
static struct fixed fixed_of(struct walk *k)
{
    struct fixed f;
    memset(&f, 0, sizeof(f));
    f.sb_size = k->sb->size, f.mss = k->sv.mss, f.eff_mss = k->sv.eff_mss;
    f.state = k->st.state, f.saw_ts = k->st.saw_timestamp, f.wscale = k->sv.wscale_peer;
    f.has_sndbuf = k->sv.sndbuf != NULL;
    return f;
}

/* One walk of family `fam`:
 *   0 cumulative ACKs through slow start into congestion avoidance
 *   1 duplicate-ACK runs of 1-6, then an ACK above snd_nxt
 *   2 the three clauses of the window update, with and without the write event
 *   3 the edges: beyond the buffer, old, no ACK flag, not valid, no timestamp
 *   4 a full send buffer, the RTO list, all data acknowledged and not
 *   5 no send buffer; an empty one with snd_nxt behind its head */
static void make_walk(int fam)
{
    static mtcp_manager_t mtcp;
    static sb_manager_t sbm;
    if (!mtcp) {
        mtcp = calloc(1, sizeof(*mtcp));
        mtcp->rbm_rcv = RBManagerCreate(RB_SIZE, 8);
        mtcp->rbm_snd = sbm = SBManagerCreate(SB_SIZE, 8);
        mtcp->rto_store = InitRTOHashstore();
        if (!mtcp->rbm_rcv || !sbm || !mtcp->rto_store) abort();
    }
    struct walk k;
    memset(&k, 0, sizeof(k));
    k.mtcp = mtcp;
    tcp_stream *st = &k.st;
    st->rcvvar = &k.rv, st->sndvar = &k.sv;
    st->state = TCP_ST_ESTABLISHED;
    st->on_rto_idx = -1;
    const int saw_ts = below(2);
    st->saw_timestamp = saw_ts;
    pthread_spin_init(&k.rv.read_lock, PTHREAD_PROCESS_PRIVATE);
    pthread_spin_init(&k.sv.write_lock, PTHREAD_PROCESS_PRIVATE);

    /* the receive side: an in-order stream into a real ring buffer */
    const uint32_t irs = below(3) == 0 ? 0xFFFFFFFFu - below(3000) : rnd();
    k.rv.irs = irs, st->rcv_nxt = irs + 1, k.rv.rcv_wnd = RB_SIZE;
    uint32_t ts_val = rnd();
    k.rv.ts_recent = ts_val;

    /* the send side */
    const uint32_t iss = below(3) == 0 ? 0xFFFFFFFFu - below(20000) : rnd();
    const uint16_t mss = below(4) == 0 ? 536 : 1460;
    k.sv.mss = mss, k.sv.eff_mss = saw_ts ? mss - 12 : mss;
    k.sv.wscale_peer = below(3) == 0 ? 0 : below(8);
    k.sb = SBInit(sbm, iss + 1);
    if (!k.sb) abort();
    k.sv.sndbuf = k.sb;
    uint32_t queued = fam == 4 ? SB_SIZE : 4000 + below(50000);  /* bytes in the send buffer */
    if (fam == 5 && below(2)) queued = 0;
    k.sb->len = queued, k.sb->tail_off = queued;
    uint32_t sent = queued ? queued - (below(3) == 0 ? below(queued) : 0) : 0;      /* of which sent */
    k.sv.snd_una = iss + 1, st->snd_nxt = iss + 1 + sent;
    if (fam == 5 && queued == 0) st->snd_nxt = iss + 1 - 1 - below(3000);             /* behind the buffer's head */
    k.sv.snd_wnd = SB_SIZE - queued;
    uint16_t window = 200 + below(60000);
    k.sv.peer_wnd = (uint32_t)window << k.sv.wscale_peer;
    if (fam == 2 && below(2)) k.sv.peer_wnd = below(sent + 1);                      /* below what is outstanding */
    k.rv.snd_wl1 = irs + 1 - below(2), k.rv.snd_wl2 = iss + 1, k.rv.last_ack_seq = iss + 1;
    k.sv.cwnd = mss * (fam == 0 ? 1 + below(3) : 2 + below(40));
    k.sv.ssthresh = fam == 0 ? mss * (4 + below(8)) : below(2) ? mss * (2 + below(30)) : 0x7FFFFFFFu;
    k.sv.rto = 1 + below(300), k.sv.ts_rto = rnd();
    if (below(2)) {                                              /* an estimate exists */
        k.rv.srtt = 8 + below(2000), k.rv.mdev = below(300);
        k.rv.mdev_max = k.rv.mdev + below(50), k.rv.rttvar = k.rv.mdev_max + below(50);
    }
    k.rv.rtt_seq = below(2) ? iss + 1 - 1 - below(1000) : iss + 1 + below(queued + 1000);   /* passed, or not yet */
    /* tcp_in.c:406 ends a run at three (snd_nxt falls to the ACK): longer runs start from a count already there */
    k.rv.dup_acks = fam != 1 ? 0 : below(4) == 0 ? 250 + below(6) : below(3) == 0 ? 2 + below(4) : 0;
    k.sv.nrtx = below(4) == 0 ? (below(2) ? 16 : below(16)) : 0;
    if (below(2)) {
        k.sv.ts_rto = 5000 + below(100);
        AddtoRTOList(mtcp, st);
        if (st->on_rto_idx < 0) abort();
    }
    if (fam == 5 && queued != 0) k.sv.sndbuf = NULL;

    /* the state record before the first packet */
    write_words(&k);
    w32(SB_SIZE), w16(k.sv.mss), w16(k.sv.eff_mss);
    w8(st->state), w8(st->saw_timestamp), w8(k.sv.wscale_peer), w8(k.rv.dup_acks);
    w8(k.sv.nrtx), w8(st->on_rto_idx >= 0), w8(k.sv.sndbuf != NULL), w8(0);
    w32((uint32_t)fam), w32(PKTS);

    uint32_t cur_ts = 6000 + below(1000);
    int dup_left = 0;
    uint32_t dup_ack = 0;
    for (int i = 0; i < PKTS; i++) {
        uint8_t hdr[64];
        struct tcphdr *tcph = (struct tcphdr *)hdr;
        memset(hdr, 0, sizeof(hdr));
        const uint32_t head = k.sb->head_seq, len = k.sb->len;
        uint32_t seq = st->rcv_nxt, ack_seq, plen = 0;
        int has_ack = 1, has_ts = 1;
        cur_ts += below(40);
        uint32_t ts_ref = cur_ts - (below(3) == 0 ? 0 : below(4) == 0 ? 500 + below(3000) : below(60));
        ts_val += below(3);
        const uint32_t step = len ? 1 + below(len < 3u * mss ? len : 3u * mss) : 0;
        ack_seq = head + step;                                  /* new data, unless the buffer is empty */
        const uint32_t r = below(100);
        if (dup_left > 0) {                                     /* a run of duplicates */
            ack_seq = dup_ack, dup_left--;
        } else if (fam == 0) {
            if (r < 8) plen = 1 + below(400);
        } else if (fam == 1) {
            if (r < 45 && TCP_SEQ_LT(k.rv.last_ack_seq, st->snd_nxt))
                dup_ack = ack_seq = k.rv.last_ack_seq, dup_left = (int)below(6);    /* 1-6 of them */
            else if (r < 55) ack_seq = head + len;              /* all of it: above snd_nxt behind a fast retransmit */
            else if (r < 60) plen = 1 + below(200);
        } else if (fam == 2) {
            ack_seq = r < 70 ? k.rv.snd_wl2 : ack_seq;          /* the same ACK: the window alone decides */
            if (r < 25) window = (uint16_t)(window + 1 + below(500));               /* snd_wl2 == ack_seq, larger */
            else if (r < 40) window = (uint16_t)(window > 600 ? window - 1 - below(500) : window);
            else if (r < 55) plen = 1 + below(300);             /* seq moves: snd_wl1 < seq */
            else if (r < 70) window = (uint16_t)(200 + below(60000));
            else if (r < 85) window = (uint16_t)(window + below(3));                /* snd_wl1 == seq, snd_wl2 < ack_seq */
        } else if (fam == 3) {
            if (r < 12) ack_seq = head + len + 1 + below(3000);                     /* beyond the buffer */
            else if (r < 24) ack_seq = head - below(3000);                          /* old */
            else if (r < 32) has_ack = 0;
            else if (r < 42) seq = st->rcv_nxt + k.rv.rcv_wnd + 1 + below(5000), plen = 1 + below(100);   /* not valid */
            else if (r < 48) seq = st->rcv_nxt - 1;                                  /* a window probe */
            else if (r < 54) has_ts = 0;                                            /* PAWS finds no timestamp */
            else if (r < 66) plen = 1 + below(700);
        } else if (fam == 4) {
            if (r < 25) ack_seq = head + len;                   /* everything acknowledged */
            else if (r < 35) ack_seq = head;
        } else {
            if (r < 30) ack_seq = head;                         /* at the head of an empty buffer, above snd_nxt */
            else if (r < 40) ack_seq = head - below(100);
        }
        tcph->seq = htonl(seq), tcph->ack_seq = htonl(ack_seq), tcph->window = htons(window);
        tcph->ack = has_ack, tcph->doff = 5;
        if (has_ts) {                                           /* NOP NOP TS, as tcp_out.c writes them */
            uint8_t *o = hdr + 20;
            uint32_t v = htonl(ts_val), e = htonl(ts_ref);
            o[0] = 1, o[1] = 1, o[2] = 8, o[3] = 10;
            memcpy(o + 4, &v, 4), memcpy(o + 8, &e, 4);
            tcph->doff = 8;
        }
        const struct fixed before = fixed_of(&k);
        const int on_rto_before = st->on_rto_idx >= 0;
        const int cnt_before = mtcp->rto_list_cnt;
        n_wev_wnd = n_wev_room = n_add_send = n_rm_send = n_ack = n_read = 0;
        sb_len_at_entry = len;
        int ret = ValidateSequence(mtcp, st, cur_ts, tcph, seq, ack_seq, (int)plen);
        if (ret)
            Handle_TCP_ST_ESTABLISHED(mtcp, cur_ts, st, tcph, seq, ack_seq, payload, (int)plen, window);
        const struct fixed after = fixed_of(&k);
        if (memcmp(&before, &after, sizeof(before))) abort();
        /* timer.c:157-166: UpdateRetransmissionTimer ran iff SBRemove did (tcp_in.c:511, :527) */
        const int ran = k.sb->len != len, on_rto_after = st->on_rto_idx >= 0;
        const unsigned rto_rm = ran && on_rto_before, rto_add = ran && on_rto_after;
        if (!ran && on_rto_after != on_rto_before) abort();
        if (mtcp->rto_list_cnt - cnt_before != (int)rto_add - (int)rto_rm) abort();

        w32(seq), w32(ack_seq), w32(ts_ref), w32(cur_ts), w16(window), w16((uint16_t)plen);
        w8((uint8_t)has_ack), w8((uint8_t)has_ts), w8((uint8_t)(int8_t)ret), w8(0);
        w8((uint8_t)n_wev_wnd), w8((uint8_t)n_wev_room), w8((uint8_t)n_add_send), w8((uint8_t)n_rm_send);
        w8((uint8_t)rto_rm), w8((uint8_t)rto_add), w16(0);
        w32(len - (uint32_t)k.sb->len);
        write_words(&k);
        w8(k.rv.dup_acks), w8(k.sv.nrtx), w8((uint8_t)on_rto_after), w8(0);
    }
    if (st->on_rto_idx >= 0) RemoveFromRTOList(mtcp, st);
    if (k.rv.rcvbuf) RBFree(mtcp->rbm_rcv, k.rv.rcvbuf);
    SBFree(sbm, k.sb);
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s OUT WALKS\n", argv[0]);
        return 2;
    }
    const uint32_t walks = (uint32_t)atoi(argv[2]);
    out = fopen(argv[1], "wb");
    if (!out) return 1;
    w32(0x574B4341u), w32(1), w32(walks), w32(PKTS);
    for (uint32_t w = 0; w < walks; w++) make_walk((int)(w % 6));
    return fclose(out) ? 1 : 0;
}
