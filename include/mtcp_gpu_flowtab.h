/*
 * mtcp_gpu_flowtab.h — a device-resident mirror of the flow table and batch
 * StreamHTSearch behind the rx launch.
 *
 * After both checksums pass, ProcessTCPPacket forms the stream key and calls
 * StreamHTSearch(mtcp->tcp_flow_table, &s_stream) (mtcp/src/tcp_in.c:1181-1186,
 * mtcp/src/fhash.c:103-121): HashFlow names the bin (tcp_stream.c:56-90), the
 * bin's TAILQ is walked and compared with EqualFlow (tcp_stream.c:92-102).
 * The rx entry points of mtcp_gpu.h already compute the bin; the entry points
 * here answer the search itself for a whole batch: one stream id per record,
 * MTCP_GPU_FLOW_MISS where the reference would go on to CreateNewFlowHTEntry
 * (tcp_in.c:1188), MTCP_GPU_FLOW_NONE where it never reaches the table.
 *
 * The host's table stays the truth.  The device holds a MIRROR that the
 * caller keeps in step: every StreamHTInsert / StreamHTRemove of the host
 * (fhash.c:68-101) goes into a delta list, and the list is applied with one
 * mtcp_gpu_flowtab_update[_dev] per batch.
 *
 * The table.  cap = 2^cap_log2 slots of 16 B, open addressing with linear
 * probing.  A slot holds a struct mtcp_gpu_flow_entry: the 12 bytes HashFlow
 * reads, in the STREAM's orientation and as in memory (saddr = iph->daddr,
 * daddr = iph->saddr, sport = tcph->dest, dport = tcph->source: the layout of
 * a tests/golden/flow_cases.bin key), and id, the caller's stream number,
 * at most MTCP_GPU_FLOWTAB_MAX_ID.  The home slot of a key is
 * mtcp_gpu_flowtab_home: the 32-bit Jenkins value of HashFlow before its mask,
 * reduced to cap_log2 bits, so its low 17 bits are HashFlow's bin.
 *
 * The contract.  A lookup's answer is a pure function of the multiset of live
 * (key, id) pairs: a key held more than once answers with the LOWEST id.  The
 * reference would answer with the earliest inserted; but it never holds a key
 * twice: CreateNewFlowHTEntry runs only after a failed search
 * (tcp_in.c:1186-1188), and active opens draw unique tuples from the address
 * pool (addr_pool.c:103-180).  On every table without duplicate keys the two
 * rules agree (tests/test_flowtab_model.py).
 *
 * Ordering.  Updates and lookups are ordered by the stream they are issued
 * on.  A lookup must not overlap an update of the same table, nor two updates
 * each other; any number of lookups may overlap.
 *
 * Parity rests on tests/flowtab_model.py, a literal restatement of fhash.c,
 * and on the golden HashFlow values (tests/golden/flow_cases.bin,
 * rx_flowbins.bin) — NOT on reference output of StreamHTSearch: the reference
 * build under oracle/_ref interposes that symbol.
 *
 * Plain C, as mtcp_gpu.h; MTCP_GPU_ABI_VERSION is unchanged (nothing that
 * exists changes): test for MTCP_GPU_HAS_FLOWTAB.
 */
#ifndef MTCP_GPU_FLOWTAB_H
#define MTCP_GPU_FLOWTAB_H

#include "mtcp_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MTCP_GPU_HAS_FLOWTAB            1
#define MTCP_GPU_FLOW_MISS              0xFFFFFFFEu   /* TCP_OK, key not in the table */
#define MTCP_GPU_FLOWTAB_MAX_ID         0xFFFFFFEFu
#define MTCP_GPU_FLOWTAB_MIN_CAP_LOG2   4u
#define MTCP_GPU_FLOWTAB_MAX_CAP_LOG2   26u
#define MTCP_GPU_FLOWTAB_MAX_BATCH      (1u << 26)    /* records or delta entries per call */

typedef struct mtcp_gpu_flowtab mtcp_gpu_flowtab;

/* One (key, id) pair, and one slot of the table. */
typedef struct mtcp_gpu_flow_entry {
    uint32_t saddr;     /* the stream's saddr: iph->daddr of its incoming packets */
    uint32_t daddr;
    uint16_t sport;     /* the stream's sport: tcph->dest of its incoming packets */
    uint16_t dport;
    uint32_t id;        /* <= MTCP_GPU_FLOWTAB_MAX_ID */
} mtcp_gpu_flow_entry;

typedef struct mtcp_gpu_flowtab_counters {
    uint32_t live;            /* pairs held */
    uint32_t tombs;           /* removed slots not yet reused (rehash clears them) */
    uint32_t insert_failed;   /* inserts that found no slot in cap probes, or carried an id above MAX_ID */
    uint32_t remove_missed;   /* removes that found no slot with their key and id */
} mtcp_gpu_flowtab_counters;

/*
 * The home slot of a 12-byte key in a table of 2^cap_log2 slots: HashFlow's
 * Jenkins value (tcp_stream.c:56-90) before the mask, its low cap_log2 bits.
 * Host only, needs no GPU; 0xFFFFFFFF for a NULL key or cap_log2 out of range.
 */
uint32_t mtcp_gpu_flowtab_home(const void *key12, uint32_t cap_log2);

/*
 * CreateHashtable (fhash.c:16-56) for the mirror: an empty table of
 * 2^cap_log2 slots (4 .. 26) bound to ctx, on ctx's device.  Its memory comes
 * from the library's parked buffers; the call waits, within the context's wait
 * limit, for the slots to be cleared.  Destroy the table before closing its
 * context, with no launch on it in flight (DestroyHashtable, fhash.c:58-66).
 */
int mtcp_gpu_flowtab_create(mtcp_gpu_ctx *ctx, uint32_t cap_log2, mtcp_gpu_flowtab **tab);
void mtcp_gpu_flowtab_destroy(mtcp_gpu_flowtab *tab);
uint32_t mtcp_gpu_flowtab_capacity(const mtcp_gpu_flowtab *tab);

/*
 * StreamHTRemove (fhash.c:89-101) for d_del[0 .. n_del), then StreamHTInsert
 * (fhash.c:68-87) for d_ins[0 .. n_ins): all removes first.  A remove releases
 * one slot with equal key AND id.  Asynchronous on `stream` (NULL = the
 * context's stream); allocates nothing, waits for nothing, copies nothing to
 * the host, so it can sit in a stream capture.  Failures are counted in the
 * table's stats: an insert into a full table or with an id above
 * MTCP_GPU_FLOWTAB_MAX_ID (insert_failed), a remove of an absent pair
 * (remove_missed).
 * MTCP_GPU_EINVAL: tab NULL, a NULL array with a non-zero count, an array not
 * 16 B aligned, a count above MTCP_GPU_FLOWTAB_MAX_BATCH.  MTCP_GPU_EIO on an
 * abandoned context.  n_del == n_ins == 0 is MTCP_GPU_OK without a launch.
 */
int mtcp_gpu_flowtab_update_dev(mtcp_gpu_flowtab *tab, const mtcp_gpu_flow_entry *d_del, uint32_t n_del,
                                const mtcp_gpu_flow_entry *d_ins, uint32_t n_ins, void *stream);

/*
 * StreamHTSearch (tcp_in.c:1181-1186, fhash.c:103-121) for n device-resident
 * 40 B rx records: d_sid[i] = the lowest id held under record i's stream key,
 * MTCP_GPU_FLOW_MISS for a TCP_OK record whose key is not held,
 * MTCP_GPU_FLOW_NONE for every other verdict.  d_bins, when not NULL, is
 * written as mtcp_gpu_flow_hash_dev writes it.  Asynchronous, under the rules
 * of mtcp_gpu_flowtab_update_dev.
 * MTCP_GPU_EINVAL: NULL tab, d_res or d_sid (with n != 0), d_res not 8 B or
 * d_sid / d_bins not 4 B aligned, n above MTCP_GPU_FLOWTAB_MAX_BATCH, a
 * context opened with MTCP_GPU_F_COMPACT (16 B records carry no addresses).
 * MTCP_GPU_EIO on an abandoned context.  n == 0 is MTCP_GPU_OK, no launch.
 */
int mtcp_gpu_flowtab_lookup_dev(mtcp_gpu_flowtab *tab, const mtcp_gpu_result *d_res, uint32_t n,
                                uint32_t *d_sid, uint32_t *d_bins, void *stream);

/*
 * The same two calls for arrays in host memory (fhash.c:68-101;
 * tcp_in.c:1181-1186, fhash.c:103-121).  Synchronous, on the context's stream,
 * built like mtcp_gpu_flow_hash.  Bounded by the context's wait limit
 * (mtcp_gpu_set_wait_limit): past it nothing of the caller's is written,
 * MTCP_GPU_ETIMEDOUT is returned and the context is ABANDONED.
 * mtcp_gpu_flowtab_update also answers MTCP_GPU_EINVAL, before anything is
 * launched, when an entry carries an id above MTCP_GPU_FLOWTAB_MAX_ID.
 * bins may be NULL.
 */
int mtcp_gpu_flowtab_update(mtcp_gpu_flowtab *tab, const mtcp_gpu_flow_entry *del, uint32_t n_del,
                            const mtcp_gpu_flow_entry *ins, uint32_t n_ins);
int mtcp_gpu_flowtab_lookup(mtcp_gpu_flowtab *tab, const mtcp_gpu_result *res, uint32_t n, uint32_t *sid,
                            uint32_t *bins);

/*
 * The table's counters after everything queued on the context's stream.
 * Synchronous and bounded like the host calls above.
 */
int mtcp_gpu_flowtab_stats(mtcp_gpu_flowtab *tab, mtcp_gpu_flowtab_counters *stats);

/*
 * The live pairs go into a fresh array of the same size and the arrays are
 * swapped: tombs becomes 0 and probe chains shrink to what the live pairs
 * need (the reference's chained bins need no such step, fhash.c:89-101).  May
 * allocate; synchronous on the context's stream and bounded like the host
 * calls above.  No launch on the table may be in flight on another stream.
 */
int mtcp_gpu_flowtab_rehash(mtcp_gpu_flowtab *tab);

#ifdef __cplusplus
}
#endif

#endif /* MTCP_GPU_FLOWTAB_H */
