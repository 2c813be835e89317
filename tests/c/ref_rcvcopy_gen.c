/*
 * ref_rcvcopy_gen.c — TEST INFRASTRUCTURE ONLY: writes tests/golden/rcvcopy_cases.bin
 * with the reference's own RBPut (tests/make_rcvcopy_golden.py compiles and
 * runs it where the reference's sources are present; nothing of them is
 * copied: tcp_ring_buffer.h comes in by path, and tcp_ring_buffer.c,
 * memory_mgt.c and tcp_rb_frag_queue.c are linked).
 *
 * Each case is one stream through several batches of RBPut
 * (mtcp/src/tcp_ring_buffer.c:280-382; its byte work is :304-319), with an
 * RBRemove in front of a batch as the application reads (api.c:1130-1131), so
 * that head_offset advances and compactions occur.  The chunk is filled with
 * 0xEE behind RBInit (the reference leaves it as the pool has it).
 *
 * Byte i of packet number k (counted through the case) of case c is
 *     (c * 131 + k * 31 + i * 7 + (i >> 8)) & 0xFF:
 * a retransmission is another packet and carries other bytes.
 *
 * The file: u32 magic 'RCVC', u32 version, u32 cases; per case u32 family,
 * size, batches; per batch u32 bytes RBRemove took in front of it, u32 packets;
 * per packet u32 stream offset (cur_seq - init_seq), u32 len, i32 RBPut's
 * return; behind the batch u32 head_offset, tail_offset, last_len, head_seq -
 * init_seq, merged_len, fragments; per fragment u32 seq - init_seq, len; then
 * the size bytes of data[].  All little-endian.
 *
 * Families: 0 in order; 1 one segment in eight delayed; 2 retransmissions that
 * overlap what is there (front, middle, tail, superset); 3 an exact fit,
 * put_off + len == size at head_offset 0; 4 a compaction at head_offset 1, 15,
 * 16, 17 and size - 1.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tcp_ring_buffer.h"

static uint64_t rng_s = 0x2545F4914F6CDD1Dull;
static uint32_t rnd(void)
{
    rng_s ^= rng_s << 13, rng_s ^= rng_s >> 7, rng_s ^= rng_s << 17;
    return (uint32_t)(rng_s >> 16);
}
static uint32_t below(uint32_t n) { return rnd() % n; }

static FILE *out;
static void w32(uint32_t v) { fwrite(&v, 4, 1, out); }

#define MAXP 64
struct pkt {
    uint32_t off, len;
};

static uint32_t cur_case, serial;
static const uint32_t INIT_SEQ = 0xFFFFF000u;        /* the sequence numbers wrap inside a case */

static struct tcp_ring_buffer *rb;
static rb_manager_t rbm;
static uint32_t nxt;                                 /* stream offset of the first byte never sent */

static uint32_t head_off(void) { return rb->head_seq - INIT_SEQ; }

static void put_batch(uint32_t removed, const struct pkt *p, uint32_t np)
{
    static uint8_t data[256];
    w32(removed), w32(np);
    for (uint32_t k = 0; k < np; k++, serial++) {
        for (uint32_t i = 0; i < p[k].len; i++)
            data[i] = (uint8_t)(cur_case * 131 + serial * 31 + i * 7 + (i >> 8));
        int ret = RBPut(rbm, rb, data, p[k].len, INIT_SEQ + p[k].off);
        w32(p[k].off), w32(p[k].len), w32((uint32_t)ret);
    }
    uint32_t nf = 0;
    for (struct fragment_ctx *f = rb->fctx; f; f = f->next) nf++;
    w32(rb->head_offset), w32(rb->tail_offset), w32((uint32_t)rb->last_len), w32(head_off());
    w32((uint32_t)rb->merged_len), w32(nf);
    for (struct fragment_ctx *f = rb->fctx; f; f = f->next) w32(f->seq - INIT_SEQ), w32(f->len);
    fwrite(rb->data, 1, (size_t)rb->size, out);
}

/* New segments in order while the window has room, at most `want`; `stop_at`:
 * no segment ends beyond this stream offset. */
static uint32_t in_order(struct pkt *p, uint32_t want, uint32_t stop_at)
{
    uint32_t np = 0;
    while (np < want && nxt < stop_at) {
        uint32_t len = 1 + below(200);
        if (len > stop_at - nxt) len = stop_at - nxt;
        p[np].off = nxt, p[np].len = len, np++;
        nxt += len;
    }
    return np;
}

static uint32_t do_read(uint32_t len)
{
    return len ? (uint32_t)RBRemove(rbm, rb, len, AT_APP) : 0;
}

static void run_case(uint32_t fam, uint32_t size, uint32_t sub)
{
    struct pkt p[MAXP];
    rbm = RBManagerCreate(size, 4);
    if (!rbm) abort();
    rb = RBInit(rbm, INIT_SEQ);
    if (!rb) abort();
    memset(rb->data, 0xEE, size);
    nxt = 0, serial = 0;
    const uint32_t batches = fam == 4 ? 3 : 4 + below(3);
    w32(fam), w32(size), w32(batches);
    for (uint32_t b = 0; b < batches; b++) {
        uint32_t removed = 0, np = 0;
        const uint32_t wend = head_off() + size;     /* the window's end as a stream offset */
        if (fam == 4) {
            const uint32_t hs[5] = {1, 15, 16, 17, size - 1};
            const uint32_t h = hs[sub % 5];
            if (b == 0) {                            /* at least h bytes, merged */
                np = in_order(p, MAXP, h == size - 1 ? h : h + 40 + below(60));
            } else if (b == 1) {                     /* head_offset = h; then up to the chunk's end */
                removed = do_read(h);
                if (removed != h || rb->head_offset != h) abort();
                const uint32_t end = head_off() + size - h + below(h + 1);   /* head_offset + end_off >= size */
                np = in_order(p, MAXP - 2, end);
                if (np >= 3 && sub >= 5) {           /* a hole while the window moves: the last but one comes last */
                    struct pkt t = p[np - 2];
                    p[np - 2] = p[np - 1], p[np - 1] = t;
                }
            } else {
                removed = do_read(below((uint32_t)rb->merged_len + 1));
                np = in_order(p, 6, head_off() + size);
            }
        } else if (fam == 3) {
            if (b == 0) np = in_order(p, MAXP, size);          /* the last segment ends at size: an exact fit */
            else {
                removed = do_read(below((uint32_t)rb->merged_len + 1));
                np = in_order(p, 8, head_off() + size);
            }
        } else {
            if (b) removed = do_read(below((uint32_t)rb->merged_len + 1));
            np = in_order(p, 4 + below(9), head_off() + size);
            if (fam == 1)
                for (uint32_t k = 0; k + 1 < np; k++)
                    if (below(8) == 0) {             /* moves 1-4 places back */
                        uint32_t j = k + 1 + below(4);
                        if (j >= np) j = np - 1;
                        struct pkt t = p[k];
                        for (uint32_t q = k; q < j; q++) p[q] = p[q + 1];
                        p[j] = t;
                    }
            if (fam == 2 && np) {
                const uint32_t first = np;
                for (uint32_t k = 0; k < first && np < MAXP; k += 2) {
                    const uint32_t s = p[k].off, l = p[k].len, kind = (sub + k / 2) % 4;
                    uint32_t lo = s, hi = s + l;
                    if (kind == 0) lo = s > head_off() + 9 ? s - 1 - below(9) : head_off(), hi = s + (l + 1) / 2;   /* front */
                    else if (kind == 1) lo = s + l / 3, hi = lo + 1 + l / 3;                                    /* middle */
                    else if (kind == 2) lo = s + l / 2, hi = s + l + 1 + below(30);                               /* tail */
                    else lo = s > head_off() + 5 ? s - 1 - below(5) : head_off(), hi = s + l + 1 + below(5);    /* superset */
                    if (hi > wend) hi = wend;
                    if (hi > lo + 200) hi = lo + 200;
                    if (hi <= lo) continue;
                    p[np].off = lo, p[np].len = hi - lo, np++;
                    if (hi > nxt) nxt = hi;
                }
            }
        }
        put_batch(removed, p, np);
    }
    RBFree(rbm, rb);
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
    const uint32_t per[5] = {6, 8, 12, 4, 20};
    uint32_t cases = 0;
    for (int f = 0; f < 5; f++) cases += per[f];
    w32(0x43564352u), w32(1), w32(cases);
    for (uint32_t f = 0; f < 5; f++)
        for (uint32_t k = 0; k < per[f]; k++, cur_case++) run_case(f, sizes[(k / (f == 4 ? 5 : 1)) % 4], k);
    return fclose(out) ? 1 : 0;
}
