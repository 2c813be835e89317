/*
 * ref_rcvwalk_gen.c — TEST INFRASTRUCTURE ONLY: writes tests/golden/rcvwalk_cases.bin
 * with the reference's own receive tail (tests/make_rcvwalk_golden.py compiles
 * and runs it where the reference's sources are present; nothing of them is
 * copied: tcp_in.c comes in by path, which makes its static inline
 * ValidateSequence and Handle_TCP_ST_ESTABLISHED reachable, and tcp_util.c,
 * tcp_ring_buffer.c, memory_mgt.c and tcp_rb_frag_queue.c are linked).
 *
 * Per packet the driver does what ProcessTCPPacket does behind StreamHTSearch
 * for an ESTABLISHED stream (mtcp/src/tcp_in.c:1194-1209, :1256-1258):
 * ValidateSequence, and Handle_TCP_ST_ESTABLISHED if it returned TRUE.  Between
 * packets it may read as the application does (api.c:1130-1131: RBRemove and
 * the window update).  EnqueueACK and RaiseReadEvent are this file's: they
 * count the calls.
 *
 * The file: u32 magic 'RCVW', u32 version, u32 walks, u32 packets per walk;
 * per walk u32 irs, size, rcv_wnd, ts_recent, saw_timestamp, packets; per packet
 *   in:  u32 seq, ts_val, ts_ref; u16 len; u16 bytes the application reads first;
 *   out: i8 ValidateSequence's return, u8 ACK_OPT_NOW calls, u8 ACK_OPT_AGGREGATE
 *        calls, u8 RaiseReadEvent calls; u8 the packet carries NOP NOP TS (in);
 *        u8 fragments; u16 0; u32 rcv_nxt, rcv_wnd, head_seq, merged_len,
 *        ts_recent, ts_lastack_rcvd; per fragment u32 seq, len.
 * All little-endian.
 */
#include <arpa/inet.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include REF_TCP_IN_C

struct mtcp_config CONFIG;

static unsigned n_now, n_agg, n_read;

void EnqueueACK(mtcp_manager_t mtcp, tcp_stream *cur_stream, uint32_t cur_ts, uint8_t opt)
{
    if (opt == ACK_OPT_NOW) n_now++;
    else if (opt == ACK_OPT_AGGREGATE) n_agg++;
    else abort();
}

void RaiseReadEvent(mtcp_manager_t mtcp, tcp_stream *stream) { n_read++; }

/* ---- a small generator (its stream of numbers is not part of any contract) ---- */
static uint64_t rng_s = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    rng_s ^= rng_s << 13, rng_s ^= rng_s >> 7, rng_s ^= rng_s << 17;
    return (uint32_t)(rng_s >> 16);
}
static uint32_t below(uint32_t n) { return rnd() % n; }

#define PKTS 16
struct pkt_in {
    uint32_t seq, ts_val, ts_ref;
    uint16_t len, read;
    uint8_t has_ts;
};

static FILE *out;
static void w32(uint32_t v) { fwrite(&v, 4, 1, out); }
static void w16(uint16_t v) { fwrite(&v, 2, 1, out); }
static void w8(uint8_t v) { fwrite(&v, 1, 1, out); }

static uint8_t payload[65536];

static void run_walk(uint32_t irs, uint32_t size, uint32_t rcv_wnd, uint32_t ts_recent, int saw_ts,
                     const struct pkt_in *p, int npkt)
{
    struct mtcp_manager mtcp;
    tcp_stream st;
    struct tcp_recv_vars rv;
    struct tcp_send_vars sv;
    uint8_t hdr[64];
    memset(&mtcp, 0, sizeof(mtcp));
    memset(&st, 0, sizeof(st));
    memset(&rv, 0, sizeof(rv));
    memset(&sv, 0, sizeof(sv));
    static rb_manager_t rbm_small, rbm_large;         /* one pool per buffer size, shared by the walks */
    rb_manager_t *rbm = size == 4096 ? &rbm_small : &rbm_large;
    if (!*rbm) *rbm = RBManagerCreate(size, 64);
    if (!*rbm) abort();
    mtcp.rbm_rcv = *rbm;
    st.rcvvar = &rv, st.sndvar = &sv;
    st.state = TCP_ST_ESTABLISHED;
    st.saw_timestamp = saw_ts;
    st.rcv_nxt = irs + 1;
    rv.irs = irs, rv.rcv_wnd = rcv_wnd, rv.ts_recent = ts_recent;
    pthread_spin_init(&rv.read_lock, PTHREAD_PROCESS_PRIVATE);

    w32(irs), w32(size), w32(rcv_wnd), w32(ts_recent), w32((uint32_t)saw_ts), w32((uint32_t)npkt);
    for (int i = 0; i < npkt; i++) {
        struct tcphdr *tcph = (struct tcphdr *)hdr;
        memset(hdr, 0, sizeof(hdr));
        tcph->seq = htonl(p[i].seq);
        tcph->ack = 1;
        tcph->doff = 5;
        if (p[i].has_ts) {                           /* NOP NOP TS, as tcp_out.c writes them */
            uint8_t *o = hdr + 20;
            uint32_t v = htonl(p[i].ts_val), r = htonl(p[i].ts_ref);
            o[0] = 1, o[1] = 1, o[2] = 8, o[3] = 10;
            memcpy(o + 4, &v, 4), memcpy(o + 8, &r, 4);
            tcph->doff = 8;
        }
        if (p[i].read && rv.rcvbuf) {                /* api.c:1130-1131 */
            RBRemove(mtcp.rbm_rcv, rv.rcvbuf, p[i].read, AT_APP);
            rv.rcv_wnd = rv.rcvbuf->size - rv.rcvbuf->merged_len;
        }
        n_now = n_agg = n_read = 0;
        int ret = ValidateSequence(&mtcp, &st, 1000 + i, tcph, p[i].seq, 0, p[i].len);
        if (ret)
            Handle_TCP_ST_ESTABLISHED(&mtcp, 1000 + i, &st, tcph, p[i].seq, 0, payload, p[i].len, 1000);
        if (st.state != TCP_ST_ESTABLISHED) abort();

        w32(p[i].seq), w32(p[i].ts_val), w32(p[i].ts_ref), w16(p[i].len), w16(rv.rcvbuf ? p[i].read : 0);
        unsigned nf = 0;
        if (rv.rcvbuf)
            for (struct fragment_ctx *f = rv.rcvbuf->fctx; f; f = f->next) nf++;
        if (nf > 255) abort();
        w8((uint8_t)(int8_t)ret), w8((uint8_t)n_now), w8((uint8_t)n_agg), w8((uint8_t)n_read);
        w8(p[i].has_ts), w8((uint8_t)nf), w16(0);
        w32(st.rcv_nxt), w32(rv.rcv_wnd);
        w32(rv.rcvbuf ? rv.rcvbuf->head_seq : irs + 1), w32(rv.rcvbuf ? (uint32_t)rv.rcvbuf->merged_len : 0);
        w32(rv.ts_recent), w32(rv.ts_lastack_rcvd);
        if (rv.rcvbuf)
            for (struct fragment_ctx *f = rv.rcvbuf->fctx; f; f = f->next) w32(f->seq), w32(f->len);
    }
    if (rv.rcvbuf) RBFree(mtcp.rbm_rcv, rv.rcvbuf);
}

/* One walk of family `fam`. */
static void make_walk(int fam)
{
    struct pkt_in p[PKTS];
    memset(p, 0, sizeof(p));
    int saw_ts = below(2);
    uint32_t size = below(2) ? 4096 : 65536;
    uint32_t irs = below(3) == 0 ? 0xFFFFFFFFu - below(2000) : rnd();
    uint32_t rcv_wnd = below(4) == 0 ? 14600 : size; /* TCP_INITIAL_WINDOW before the first payload */
    uint32_t ts0 = rnd(), ts = ts0;
    uint32_t max_len = fam == 2 ? 64 : (size == 4096 ? 700 : 1460);
    /* the stream's segments, in order */
    uint32_t sseq[PKTS + 1], slen[PKTS];
    sseq[0] = irs + 1;
    for (int i = 0; i < PKTS; i++) {
        slen[i] = 1 + below(max_len);
        sseq[i + 1] = sseq[i] + slen[i];
    }
    int order[PKTS];
    for (int i = 0; i < PKTS; i++) order[i] = i;
    if (fam == 2) {                                  /* holes: the odd segments first, so the list grows past four */
        int k = 0;
        for (int i = 1; i < PKTS; i += 2) order[k++] = i;
        for (int i = 0; i < PKTS; i += 2) order[k++] = i;
    } else {                                         /* a segment in eight moves 1-8 places back */
        for (int i = 0; i < PKTS; i++)
            if (below(8) == 0) {
                int d = 1 + (int)below(8), j = i + d < PKTS ? i + d : PKTS - 1, t = order[i];
                for (int k = i; k < j; k++) order[k] = order[k + 1];
                order[j] = t;
            }
    }
    for (int i = 0; i < PKTS; i++) {
        int s = order[i];
        if (fam != 2 && i > 0 && below(16) == 0) s = order[below((uint32_t)i)];   /* an earlier one again */
        p[i].seq = sseq[s], p[i].len = (uint16_t)slen[s];
        ts += below(3);
        p[i].has_ts = 1, p[i].ts_val = ts, p[i].ts_ref = rnd();
        uint32_t r = below(100);
        if (fam == 1) {                              /* the edges */
            if (r < 6) p[i].seq += 0x80000000u;                           /* exactly 2^31 ahead */
            else if (r < 10) p[i].seq = sseq[s] + 0x80000000u - p[i].len; /* its end exactly 2^31 ahead */
            else if (r < 14) p[i].ts_val = ts + 0x80000000u;              /* a timestamp exactly 2^31 off */
            else if (r < 18) p[i].ts_val = ts - 1 - below(5);             /* stale */
            else if (r < 22) p[i].has_ts = 0;                             /* no option at all */
            else if (r < 28) p[i].len = 0;                                /* an ACK */
            else if (r < 32) p[i].seq = sseq[s] - 1, p[i].len = (uint16_t)below(2);   /* a window probe */
            else if (r < 38) p[i].len = (uint16_t)(p[i].len + 1 + below(900));    /* overlaps what follows */
            else if (r < 44) p[i].seq -= 1 + below(300), p[i].len = (uint16_t)(p[i].len + 300);   /* and what precedes */
            else if (r < 50) p[i].read = (uint16_t)(1 + below(3000));     /* the application reads */
            else if (r < 53) p[i].seq += size;                            /* beyond the buffer */
            if (i == 0 && rcv_wnd > size && below(2))                     /* inside the initial window, past the buffer */
                p[i].seq = irs + 1 + size - below(300), p[i].len = (uint16_t)(301 + below(600)), p[i].read = 0;
        } else if (fam == 0) {
            if (r < 4) p[i].read = (uint16_t)(1 + below(2000));
            else if (r < 6) p[i].has_ts = 0;
            else if (r < 8) p[i].ts_val = ts - 1 - below(5);
        }
        if (!p[i].has_ts) p[i].ts_val = p[i].ts_ref = 0;
    }
    run_walk(irs, size, rcv_wnd, ts0, saw_ts, p, PKTS);
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
    w32(0x57564352u), w32(1), w32(walks), w32(PKTS);
    for (uint32_t w = 0; w < walks; w++) make_walk(w % 8 < 3 ? 0 : w % 8 < 6 ? 1 : 2);
    return fclose(out) ? 1 : 0;
}
