/*
 * ref_rcvread_gen.c — TEST INFRASTRUCTURE ONLY: writes tests/golden/rcvread_cases.bin
 * with the reference's own ring buffer (tests/make_rcvread_golden.py compiles
 * and runs it where the reference's sources are present; nothing of them is
 * copied: tcp_ring_buffer.h comes in by path, and tcp_ring_buffer.c,
 * memory_mgt.c and tcp_rb_frag_queue.c are linked).
 *
 * What is pinned.  RBInit, RBPut and RBRemove are the reference's: the offsets,
 * head_seq, merged_len, the fragment list and the bytes a read returns are
 * theirs.  CopyToUser and PeekForUser are static inline inside mtcp/src/api.c
 * and cannot be linked; copy_to_user() and peek_for_user() below restate their
 * few lines (api.c:1114-1149, :1096-1112) around those calls, each line cited.
 * rcv_wnd after a put is tcp_in.c:589's assignment, restated likewise.
 *
 * Byte i of put number k (counted through the case) of case c is
 *     (c * 113 + k * 29 + i * 5 + (i >> 8)) & 0xFF.
 *
 * The file: u32 magic 'RCVR', u32 version, u32 cases; per case u32 family, size,
 * init_seq, eff_mss, events; per event u32 kind (0 put, 1 read, 2 peek), then
 *   put:        u32 cur_seq, len, i32 RBPut's return;
 *   read, peek: u32 len, need_wnd_adv before, on_ackq before, i32 the return
 *               value (-1: EAGAIN), u32 need_wnd_adv after, on_ackq after,
 *               whether RBRemove freed the first fragment, then the returned
 *               bytes of the user buffer, padded with zeros to 4 bytes;
 * then behind every event u32 head_offset, tail_offset, last_len, head_seq,
 * merged_len, rcv_wnd, fragments; per fragment u32 seq, len.  Little-endian.
 *
 * Families: 0 len below, equal to and above merged_len, merged_len 0 (before
 * any put and behind a hole at the head), len 1; 1 two to four fragments, a
 * read that empties the first against one that trims it; 2 reads that leave
 * head_offset at 1, 15, 16, 17 and size - 1, so that the next RBPut compacts;
 * 3 random reads, peeks and puts interleaved; 4 head_seq across 2^32; 5 rcv_wnd
 * at eff_mss - 1, eff_mss and eff_mss + 1 after the read with need_wnd_adv and
 * on_ackq each 0 and 1.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tcp_ring_buffer.h"

#define MIN(a, b) ((a) < (b) ? (a) : (b))

static uint64_t rng_s = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    rng_s ^= rng_s << 13, rng_s ^= rng_s >> 7, rng_s ^= rng_s << 17;
    return (uint32_t)(rng_s >> 16);
}
static uint32_t below(uint32_t n) { return rnd() % n; }

static FILE *out;
static void w32(uint32_t v) { fwrite(&v, 4, 1, out); }

static uint32_t cur_case, serial, events;
static long events_at;

static struct tcp_ring_buffer *rb;
static rb_manager_t rbm;
static uint32_t init_seq, nxt;                      /* nxt: sequence number of the first byte never sent */
/* the fields of tcp_stream, tcp_recv_vars and tcp_send_vars the two functions touch */
static uint32_t rcv_wnd, eff_mss;
static uint8_t need_wnd_adv, on_ackq;

static void snapshot(void)
{
    uint32_t nf = 0;
    for (struct fragment_ctx *f = rb->fctx; f; f = f->next) nf++;
    w32(rb->head_offset), w32(rb->tail_offset), w32((uint32_t)rb->last_len), w32(rb->head_seq);
    w32((uint32_t)rb->merged_len), w32(rcv_wnd), w32(nf);
    for (struct fragment_ctx *f = rb->fctx; f; f = f->next) w32(f->seq), w32(f->len);
    events++;
}

static void put(uint32_t seq, uint32_t len)
{
    static uint8_t data[4096];
    for (uint32_t i = 0; i < len; i++) data[i] = (uint8_t)(cur_case * 113 + serial * 29 + i * 5 + (i >> 8));
    serial++;
    int ret = RBPut(rbm, rb, data, len, seq);
    rcv_wnd = rb->size - rb->merged_len;             /* tcp_in.c:589 */
    w32(0), w32(seq), w32(len), w32((uint32_t)ret);
    snapshot();
}

/* in order: the next len bytes */
static void put_next(uint32_t len)
{
    put(nxt, len);
    nxt += len;
}

/* PeekForUser, api.c:1096-1112 */
static int peek_for_user(char *buf, int len)
{
    int copylen;
    copylen = MIN(rb->merged_len, len);              /* api.c:1102 */
    if (copylen <= 0) return -1;                     /* api.c:1103-1106 */
    memcpy(buf, rb->head, copylen);                  /* api.c:1109 */
    return copylen;                                  /* api.c:1111 */
}

/* CopyToUser, api.c:1114-1149 */
static int copy_to_user(char *buf, int len)
{
    int copylen;
    copylen = MIN(rb->merged_len, len);              /* api.c:1121 */
    if (copylen <= 0) return -1;                     /* api.c:1122-1125 */
    memcpy(buf, rb->head, copylen);                  /* api.c:1129 */
    RBRemove(rbm, rb, copylen, AT_APP);              /* api.c:1130 */
    rcv_wnd = rb->size - rb->merged_len;             /* api.c:1131 */
    if (need_wnd_adv) {                              /* api.c:1134 */
        if (rcv_wnd > eff_mss) {                     /* api.c:1135 */
            if (!on_ackq) {                          /* api.c:1136 */
                on_ackq = 1;                         /* api.c:1138 */
                need_wnd_adv = 0;                    /* api.c:1141 */
            }
        }
    }
    return copylen;                                  /* api.c:1148 */
}

static int rd(uint32_t len, int peek)
{
    static char buf[8192];
    struct fragment_ctx *first = rb->fctx;
    w32(peek ? 2 : 1), w32(len), w32(need_wnd_adv), w32(on_ackq);
    memset(buf, 0, sizeof(buf));
    int ret = peek ? peek_for_user(buf, (int)len) : copy_to_user(buf, (int)len);
    w32((uint32_t)ret), w32(need_wnd_adv), w32(on_ackq), w32(rb->fctx != first);
    if (ret > 0) fwrite(buf, 1, ((size_t)ret + 3) & ~(size_t)3, out);
    snapshot();
    return ret;
}

static void begin(uint32_t fam, uint32_t size, uint32_t iseq, uint32_t mss)
{
    rbm = RBManagerCreate(size, 4);
    if (!rbm) abort();
    rb = RBInit(rbm, iseq);
    if (!rb) abort();
    memset(rb->data, 0xEE, size);
    init_seq = iseq, nxt = iseq, serial = 0, events = 0;
    rcv_wnd = size, eff_mss = mss, need_wnd_adv = 0, on_ackq = 0;
    w32(fam), w32(size), w32(iseq), w32(mss);
    events_at = ftell(out);
    w32(0);
}

static void end(void)
{
    const long here = ftell(out);
    fseek(out, events_at, SEEK_SET);
    w32(events);
    fseek(out, here, SEEK_SET);
    RBFree(rbm, rb);
    cur_case++;
}

static void fam0(uint32_t size)
{
    begin(0, size, 0x1000u + below(1u << 20), 64);
    rd(10, 0), rd(10, 1);                            /* merged_len 0: nothing was put */
    put(nxt + 40, 20);                               /* a hole at the head: merged_len stays 0 */
    rd(10, 0), rd(1, 1);
    put_next(40);                                    /* fills the hole: 60 merged */
    nxt += 20;
    rd(0, 0);                                        /* len 0 */
    rd(1, 0);                                        /* len 1 */
    rd(30, 1), rd(30, 0);                            /* below merged_len */
    rd((uint32_t)rb->merged_len, 0);                 /* equal: empties the buffer */
    rd(5, 0);
    put_next(100 + below(100));
    rd((uint32_t)rb->merged_len + 1 + below(5000), 0);   /* above */
    put_next(1);
    rd(1, 0);
    put_next(size / 2);
    rd(0x7FFFFFFFu, 1), rd(0x7FFFFFFFu, 0);
    end();
}

static void fam1(uint32_t size, uint32_t nfrag, int empties)
{
    begin(1, size, 0x40000000u + below(1u << 20), 64);
    const uint32_t flen = 24 + below(40);
    put_next(flen);                                  /* the first fragment, merged */
    for (uint32_t k = 1; k < nfrag; k++) {
        nxt += 8 + below(8);                         /* a hole in front of each further one */
        put_next(16 + below(32));
    }
    rd(3, 1);
    if (empties) rd(flen, 0);                        /* :403-411 */
    else rd(flen - 1 - below(flen - 1), 0);          /* :412-415 */
    rd(4, 1);
    rd(flen, 0);
    rd(1, 0);
    end();
}

static void fam2(uint32_t size, uint32_t h)
{
    begin(2, size, 0x7FFFF000u + below(4096), 64);
    if (h == size - 1) {
        put_next(size / 2), put_next(size - size / 2);
    } else {
        put_next(h + 50 + below(50));
    }
    rd(h, 0);                                        /* head_offset == h */
    if (rb->head_offset != h) abort();
    rd(7, 1);
    /* up to the chunk's end: head_offset + end_off >= size, RBPut compacts */
    while (rb->head_offset != 0) put_next(MIN(200, size - (nxt - rb->head_seq)));
    rd(33, 0);
    put_next(10);
    rd(0x10000, 0);
    end();
}

static void fam3(uint32_t size)
{
    begin(3, size, below(0xFFFFFFFFu), 1 + below(size));
    const uint32_t steps = 24 + below(16);
    for (uint32_t s = 0; s < steps; s++) {
        const uint32_t k = below(8);
        const uint32_t room = size - (nxt - rb->head_seq);
        if (k < 3 && room) {
            put_next(1 + below(MIN(room, 300)));
        } else if (k == 3 && room > 40) {            /* out of order: a hole, filled by the next in-order put or not */
            const uint32_t gap = 1 + below(16), len = 1 + below(MIN(room - gap - 1, 100));
            put(nxt + gap, len);
        } else if (k == 4) {
            need_wnd_adv = (uint8_t)below(2), on_ackq = (uint8_t)below(2);
            rd(below((uint32_t)rb->merged_len + 40), 1);
        } else {
            need_wnd_adv = (uint8_t)below(2), on_ackq = (uint8_t)below(2);
            rd(below(3) ? below((uint32_t)rb->merged_len + 40) : 1 + below(8), 0);
        }
    }
    end();
}

static void fam4(uint32_t size, uint32_t back)
{
    begin(4, size, 0u - back, 64);                   /* head_seq wraps inside the case */
    for (uint32_t s = 0; s < 10; s++) {
        put_next(MIN(120, size - (nxt - rb->head_seq)));
        if (s == 2) put(nxt + 10, 30);
        rd(s & 1 ? 1000 : 50 + below(60), s == 4);
    }
    end();
}

/* rcv_wnd after the read at eff_mss + delta - 1 for delta 0, 1, 2 */
static void fam5(uint32_t size, uint32_t delta, uint32_t nwa, uint32_t ackq)
{
    const uint32_t mss = size / 2;
    begin(5, size, 0x20000000u, mss);
    put_next(size / 2), put_next(size - size / 2);   /* full: rcv_wnd 0, the reference sets need_wnd_adv when it
                                                        advertises that (tcp_out.c:301-306) */
    need_wnd_adv = (uint8_t)nwa, on_ackq = (uint8_t)ackq;
    rd(5, 1);
    rd(mss + delta - 1, 0);                          /* merged_len = size - that: rcv_wnd = mss + delta - 1 */
    rd(1, 0);
    rd(1, 0);
    end();
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: %s OUT\n", argv[0]);
        return 2;
    }
    out = fopen(argv[1], "wb");
    if (!out) return 1;
    const uint32_t sizes[4] = {256, 512, 1024, 2048};
    w32(0x52564352u), w32(1), w32(0);
    for (uint32_t k = 0; k < 4; k++) fam0(sizes[k]);
    for (uint32_t nf = 2; nf <= 4; nf++)
        for (int e = 0; e < 2; e++) fam1(sizes[nf % 4], nf, e);
    for (uint32_t k = 0; k < 10; k++) {
        const uint32_t size = sizes[k % 4], hs[5] = {1, 15, 16, 17, size - 1};
        fam2(size, hs[k % 5]);
    }
    for (uint32_t k = 0; k < 24; k++) fam3(sizes[k % 4]);
    for (uint32_t k = 0; k < 4; k++) fam4(sizes[k], 1 + below(300));
    for (uint32_t d = 0; d < 3; d++)
        for (uint32_t f = 0; f < 4; f++) fam5(sizes[(d + f) % 4], d, f & 1, f >> 1);
    fseek(out, 8, SEEK_SET);
    w32(cur_case);
    return fclose(out) ? 1 : 0;
}
