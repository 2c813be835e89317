/*
 * ref_sndwrite_gen.c — TEST INFRASTRUCTURE ONLY: writes tests/golden/sndwrite_cases.bin
 * with the reference's own send buffer (tests/make_sndwrite_golden.py compiles
 * and runs it where the reference's sources are present; nothing of them is
 * copied: tcp_send_buffer.h comes in by path, and tcp_send_buffer.c,
 * memory_mgt.c and tcp_sb_queue.c are linked).
 *
 * What is pinned.  SBManagerCreate, SBInit, SBPut and SBRemove are the
 * reference's: the return values, head_off, tail_off, len, cum_len, head_seq and
 * every byte of the chunk after every operation are theirs.  The chunk is filled
 * with 0xEE behind SBInit, so that bytes no operation wrote are told apart.
 *
 * Byte i of put number k (counted through the case, refused puts included) of
 * case c is (c * 113 + k * 29 + i * 5 + (i >> 8)) & 0xFF.
 *
 * The file: u32 magic 'SNDW', u32 version, u32 cases; per case u32 family, size,
 * init_seq, operations; per operation u32 kind (0 SBPut, 1 SBRemove), u32 len,
 * i32 the return value, u32 head_off, tail_off, len, cum_len (low, high),
 * head_seq, then the size bytes of data[].  Sizes are multiples of 4.
 * Little-endian.
 *
 * Families: 0 puts that fit below size, len 1, the exact fit with head_off 0 (a
 * move onto itself), a put clamped by size - len, a put into a full buffer
 * (-2); 1 the exact fit with head_off > 0; 2 compaction at head_off 1, 15, 16,
 * 17 and size - 1; 3 moved lengths 1, 15, 16, 17 and around 1 024 and 2 048; 4 a
 * put whose destination after the move overlaps the old window; 5 a remove
 * that empties the buffer and resets the offsets, followed by a put; 6 puts
 * and removes interleaved over many rounds; 7 head_seq across 2^32.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tcp_send_buffer.h"

static uint64_t rng_s = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    rng_s ^= rng_s << 13, rng_s ^= rng_s >> 7, rng_s ^= rng_s << 17;
    return (uint32_t)(rng_s >> 16);
}
static uint32_t below(uint32_t n) { return rnd() % n; }

static FILE *out;
static void w32(uint32_t v) { fwrite(&v, 4, 1, out); }

static uint32_t cases, cur_case, serial, ops;
static long cases_at, ops_at;
static sb_manager_t sbm;
static struct tcp_send_buffer *sb;

static void begin(uint32_t family, uint32_t size, uint32_t init_seq)
{
    sbm = SBManagerCreate(size, 1);
    sb = sbm ? SBInit(sbm, init_seq) : NULL;
    if (!sb) {
        fprintf(stderr, "no send buffer of %u bytes\n", size);
        exit(1);
    }
    memset(sb->data, 0xEE, size);
    cur_case = cases++, serial = 0, ops = 0;
    w32(family), w32(size), w32(init_seq);
    ops_at = ftell(out);
    w32(0);
}

static void end(void)
{
    const long at = ftell(out);
    fseek(out, ops_at, SEEK_SET), w32(ops), fseek(out, at, SEEK_SET);
}

static void snapshot(uint32_t kind, uint32_t len, long ret)
{
    w32(kind), w32(len), w32((uint32_t)(int32_t)ret);
    w32(sb->head_off), w32(sb->tail_off), w32(sb->len), w32((uint32_t)sb->cum_len), w32((uint32_t)(sb->cum_len >> 32));
    w32(sb->head_seq);
    fwrite(sb->data, 1, sb->size, out);
    ops++;
}

static long put(uint32_t len)
{
    static uint8_t data[16384];
    for (uint32_t i = 0; i < len; i++) data[i] = (uint8_t)(cur_case * 113 + serial * 29 + i * 5 + (i >> 8));
    serial++;
    const long ret = (long)SBPut(sbm, sb, data, len);
    snapshot(0, len, ret);
    return ret;
}

static long rem(uint32_t len)
{
    const long ret = (long)SBRemove(sbm, sb, len);
    snapshot(1, len, ret);
    return ret;
}

int main(int argc, char **argv)
{
    if (argc != 2 || !(out = fopen(argv[1], "wb"))) return 1;
    w32(0x57444E53u), w32(1);
    cases_at = ftell(out);
    w32(0);

    /* 0: below size, len 1, the exact fit at head_off 0, clamped, full */
    begin(0, 64, 1000), put(1), put(15), put(16), put(17), put(14), put(1), put(1), end();            /* 63, then 64: -2 */
    begin(0, 48, 77), put(47), put(1), put(5), end();                       /* the exact fit moves 47 bytes onto themselves */
    begin(0, 128, 5), put(100), put(100), put(1), end();                    /* clamped to 28 (an exact fit), then -2 */
    begin(0, 256, 9), put(256), put(3), end();                              /* one put fills it */
    begin(0, 96, 3), put(40), put(40), put(15), put(1), put(1), end();      /* 95, the exact fit, -2 */
    /* 1: the exact fit with head_off > 0 */
    for (uint32_t h = 1; h <= 33; h += 8) begin(1, 128, 4000 + h), put(90), rem(h), put(38), put(h), end();
    /* 2: compaction at head_off 1, 15, 16, 17, size - 1 */
    {
        const uint32_t hs[] = {1, 15, 16, 17};
        for (int k = 0; k < 4; k++)
            for (uint32_t size = 64; size <= 192; size += 128)
                begin(2, size, 100 * k + size), put(size - 8), rem(hs[k]), put(30), put(size), end();
        begin(2, 64, 8), put(64), rem(63), put(10), put(64), end();          /* head_off size - 1: one byte moves */
        begin(2, 512, 8), put(512), rem(511), put(500), put(64), end();
    }
    /* 3: moved lengths */
    {
        const uint32_t ms[] = {1, 15, 16, 17};
        for (int k = 0; k < 4; k++)                                             /* window ms[k] long at head_off 40 + k */
            begin(3, 128, 900 + k), put(40 + k + ms[k]), rem(40 + k), put(100), end();
        for (uint32_t m = 1023; m <= 1025; m++) begin(3, 4096, m), put(m + 3000), rem(3000), put(200), end();
        for (uint32_t m = 2047; m <= 2049; m++) begin(3, 4096, m), put(m + 1999), rem(1999), put(100), end();
        begin(3, 8192, 1), put(8000), rem(5951), put(4000), end();              /* 2 049 bytes down by 5 951 */
        begin(3, 8192, 2), put(8192), rem(7168), put(8192), end();              /* 1 024 bytes, then a clamped put */
    }
    /* 4: the destination after the move overlaps the old window */
    begin(4, 256, 31), put(200), rem(3), put(59), end();                       /* [197, 256) inside the old [3, 200) */
    begin(4, 256, 32), put(250), rem(100), put(106), end();                    /* [150, 256) over the old [100, 250) */
    begin(4, 512, 33), put(500), rem(17), put(29), put(1), end();
    /* 5: a remove that empties the buffer, then a put */
    begin(5, 128, 600), put(70), rem(70), put(20), rem(20), put(128), rem(128), put(1), end();
    begin(5, 64, 601), put(10), rem(4), rem(100), put(60), rem(0), end();       /* a remove clamped by len */
    /* 6: interleaved over many rounds */
    for (int c = 0; c < 6; c++) {
        const uint32_t size = 48 + 16 * below(12);
        begin(6, size, rnd());
        for (int r = 0; r < 40; r++) {
            if (below(3)) put(1 + below(below(4) ? size / 3 : size + 8));
            else rem(below(4) ? 1 + below(size / 2) : sb->len);
        }
        end();
    }
    /* 7: head_seq across 2^32 */
    begin(7, 128, 0xFFFFFFC0u), put(100), rem(30), rem(40), put(90), rem(60), put(70), end();
    begin(7, 64, 0xFFFFFFFFu), put(10), rem(1), put(54), rem(9), put(10), end();

    const long at = ftell(out);
    fseek(out, cases_at, SEEK_SET), w32(cases), fseek(out, at, SEEK_SET);
    return fclose(out) ? 1 : 0;
}
