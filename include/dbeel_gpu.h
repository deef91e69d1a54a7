/* dbeel_gpu.h — C ABI of the MI355X-native SSTable compaction engine.
 *
 * This is the drop-in seam for dbeel's `LSMTree::compact` hot path
 * (reference: src/storage_engine/lsm_tree.rs:950-1156). Everything from
 * lsm_tree.rs:974 down (read -> k-way merge/dedup -> write) is replaced by
 * `dbeel_gpu_compact`; the caller keeps the reference's surrounding side
 * effects (bloom file, .compact_action journal, renames, sstable-list swap —
 * lsm_tree.rs:1070-1153).
 *
 * Wire format (all integers little-endian, bincode fixint — reference
 * src/utils/bincode.rs:9-16):
 *   entry      = key_len:u64 | key bytes | data_len:u64 | data bytes |
 *                timestamp:i128                 (src/storage_engine/mod.rs:68-73,
 *                                               src/utils/timestamp_nanos.rs:6-11)
 *   index rec  = offset:u64 | key_size:u32 | full_size:u32   = 16 bytes
 *                (src/storage_engine/mod.rs:45-50, INDEX_ENTRY_SIZE mod.rs:33,
 *                 asserted lsm_tree.rs:408-413)
 *   key_size   = 8 + key_len;  full_size = 32 + key_len + data_len
 *
 * Merge semantics (lsm_tree.rs:1038-1066, CompactionItem ordering
 * lsm_tree.rs:52-71 + Entry::cmp mod.rs:75-81):
 *   total order: key bytes ascending (lexicographic), then timestamp
 *   ascending (signed i128), then run index ascending. Among entries with
 *   equal key, exactly one survives: the max by (timestamp, run index)
 *   ("last pop of an equal-key group wins"). A surviving entry whose data is
 *   empty (TOMBSTONE, mod.rs:14) is dropped unless keep_tombstones.
 *   Survivors are emitted verbatim (input bytes unchanged) in total order,
 *   densely packed; index offsets recomputed from 0
 *   (entry_writer.rs:71-98).
 *
 * Input invariants (guaranteed by dbeel's flush/compaction writers,
 * lsm_tree.rs:925-946): each run is sorted ascending by key with unique keys
 * within the run. Corrupt inputs (index size not a multiple of 16, entry
 * ranges out of bounds, full_size < 32 + key_len) return
 * DBEEL_ERR_CORRUPT_RECORD; the reference silently treats a failed decode as
 * end-of-stream (lsm_tree.rs:1014,1063 "if let Ok"), this engine errors
 * loudly instead (documented divergence).
 */
#ifndef DBEEL_GPU_H
#define DBEEL_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One SSTable run, resident in host DRAM, caller-owned, read-only.
 * runs[] must be ordered by ascending sstable index — the (timestamp, run
 * index) tie-break depends on it (lsm_tree.rs:58-65). */
typedef struct {
    const uint8_t* data;      /* run data file bytes (concatenated entries) */
    size_t         data_len;
    const uint8_t* index;     /* run index file bytes (16-byte records)     */
    size_t         index_len;
} dbeel_run_view;

/* Engine-allocated outputs; free with dbeel_gpu_result_free. */
typedef struct {
    uint8_t* data;            /* output .data file bytes  */
    size_t   data_len;
    uint8_t* index;           /* output .index file bytes */
    size_t   index_len;
    uint64_t entries_written;
} dbeel_compact_result;

/* Optional per-call timing/throughput evidence (milliseconds, HIP events on
 * the job's stream). kernel_ms covers the whole device pipeline
 * (rank -> scan -> emit -> copy), excluding host<->device copies. */
typedef struct {
    double h2d_ms;
    double prep_ms;    /* k_prepare: validation + key-prefix/aux extract */
    double rank_ms;    /* k_corank + k_rankreduce: merge-path crossranks,
                          global ranks, winner flags                 */
    double scan_ms;    /* survivor size/position prefix sums        */
    double emit_ms;    /* output index build + survivor source map  */
    double copy_ms;    /* verbatim entry copy-out (incl. k_winmap)  */
    double kernel_ms;  /* prep+rank+scan+emit+copy                  */
    double d2h_ms;
} dbeel_compact_timings;

/* Error codes. Mirrors the reference error taxonomy at this seam
 * (src/error.rs; ItemTooLarge error.rs:60-61). */
enum {
    DBEEL_OK               = 0,
    DBEEL_ERR_INVALID_ARG  = 1,
    DBEEL_ERR_CORRUPT      = 2,  /* bincode-decode-failure analogue */
    DBEEL_ERR_ITEM_TOO_LARGE = 3,
    DBEEL_ERR_HIP          = 4,  /* device/runtime failure */
    DBEEL_ERR_NO_GPU       = 5,
    DBEEL_ERR_OOM          = 6,
    DBEEL_ERR_IO           = 7,  /* host filesystem failure (error.rs I/O
                                    analogue) — distinct from device errors */
};

/* Compact n_runs runs into one run. keep_tombstones: 0 = drop entries with
 * empty value data (lsm_tree.rs:1045-1046). device: HIP device ordinal
 * (>= 0). There is NO CPU fallback in this library: the CPU restatement
 * lives in liboracle.so (test infrastructure only) and device < 0 returns
 * DBEEL_ERR_INVALID_ARG. Returns 0 on success. Reentrant; concurrent calls
 * on distinct devices run independent jobs. */
int dbeel_gpu_compact(const dbeel_run_view* runs, size_t n_runs,
                      int keep_tombstones, int device,
                      dbeel_compact_result* out);

/* Same, and also reports timings (t may be NULL). */
int dbeel_gpu_compact_timed(const dbeel_run_view* runs, size_t n_runs,
                            int keep_tombstones, int device,
                            dbeel_compact_result* out,
                            dbeel_compact_timings* t);

void dbeel_gpu_result_free(dbeel_compact_result* r);

/* Thread-local message for the last error in this thread. */
const char* dbeel_gpu_last_error(void);

/* ---- Batched point lookup ----
 * GPU analogue of LSMTree::get over the sstables (lsm_tree.rs:674-723):
 * the reference scans sstables newest-INDEX-first and returns the first
 * key match (`sstables.iter().rev()`, lsm_tree.rs:692-696) — so the match
 * in the HIGHEST run index wins, regardless of timestamp. (This can
 * differ from the compaction winner rule when set_with_timestamp writes
 * an older timestamp into a newer sstable; compaction then reorders —
 * faithful to the reference read path.) run = -1 when absent;
 * is_tombstone = 1 distinguishes deleted from absent (the reference's
 * delete->get->KeyNotFound semantics). value_offset indexes into
 * runs[run].data. Bloom prefiltering stays host-side
 * (dbeel_bloom_contains). keys: concatenated blob + n+1 offsets. */
typedef struct {
    int32_t run;
    uint32_t is_tombstone;
    uint64_t value_offset;
    uint64_t value_len;
} dbeel_lookup_hit;

int dbeel_gpu_lookup(const dbeel_run_view* runs, size_t n_runs,
                     const uint8_t* keys, const uint64_t* key_offsets,
                     uint64_t n_keys, int device, dbeel_lookup_hit* out);

/* ---- Resident table reader (the read-path seam) ----
 * LSMTree::get over the sstables (lsm_tree.rs:674-723) with the tables
 * resident in HBM: open uploads the runs (and their "DBLM" filters,
 * format in include/dbeel_lsm.h) once; every get after that moves only
 * the query keys in and the hits + packed value bytes out.
 *
 * Results are exactly dbeel_gpu_lookup's (newest run index first, first
 * key match wins, run = -1 absent, a tombstone is found with
 * is_tombstone = 1 / value_len = 0, value_offset indexes runs[run].data);
 * the value bytes of query q are additionally delivered at
 * values[value_offsets[q] .. value_offsets[q+1]). A run that has a filter
 * is searched only when the filter answers "maybe" — the reference
 * consults each sstable's bloom inside the same newest-first loop
 * (lsm_tree.rs:692-696); the device decision equals dbeel_bloom_contains
 * on the same bytes.
 *
 * open validates arguments (runs as for jobs, n_runs <= 64, device >= 0,
 * every filter's magic/version/length — a bad filter is
 * DBEEL_ERR_CORRUPT) before any device call, then uploads, then runs a
 * device pass that validates every entry, checks that each run is
 * strictly ascending by key and builds the dense 8-byte key-prefix array
 * the search runs on; any violation is DBEEL_ERR_CORRUPT.
 *
 * A reader holds one table per run — the padded run bytes, 8 B per entry
 * of prefixes, the filter bitmap (dbeel_gpu_reader_table_bytes reports the
 * sum over its tables, a pending compaction output included) — and
 * per-batch scratch that grows on demand and is reused — no compaction
 * buffers. One thread at a time per reader; distinct readers are
 * independent. */
typedef struct {
    const uint8_t* bytes;     /* whole .bloom file; NULL = run has no filter */
    size_t         len;
} dbeel_bloom_view;

typedef struct dbeel_gpu_reader dbeel_gpu_reader;

int dbeel_gpu_reader_open(const dbeel_run_view* runs,
                          const dbeel_bloom_view* blooms /* NULL or n_runs */,
                          size_t n_runs, int device, dbeel_gpu_reader** out);
/* Device bytes held between calls: slab + prefixes + bitmaps. */
uint64_t dbeel_gpu_reader_table_bytes(const dbeel_gpu_reader* reader);

/* Engine-allocated; free with dbeel_gpu_get_result_free. */
typedef struct {
    dbeel_lookup_hit* hits;          /* n_keys                              */
    uint64_t*         value_offsets; /* n_keys+1, exclusive; absent or
                                        tombstone = empty range            */
    uint8_t*          values;        /* packed in query order               */
    uint64_t          values_len, n_keys;
} dbeel_get_result;

/* Per-call evidence. Times are HIP events on the reader's stream:
 * search_ms is the search kernel alone, gather_ms the value-offset scan
 * plus the gather kernel. bloom_probes = filter checks performed,
 * bloom_skips = checks that answered "absent", searches = binary searches
 * performed, so searches = (bloom_probes - bloom_skips) + visits to
 * unfiltered runs. hits counts found keys (tombstones included),
 * tombstones those found deleted. */
typedef struct {
    double   h2d_ms, search_ms, gather_ms, d2h_ms;
    uint64_t bloom_probes, bloom_skips, searches, hits, tombstones;
} dbeel_get_stats;

/* keys: concatenated blob + n_keys+1 ascending offsets. Zero-length and
 * duplicate keys are legal; n_keys == 0 succeeds with empty outputs. */
int dbeel_gpu_reader_get(dbeel_gpu_reader* reader, const uint8_t* keys,
                         const uint64_t* key_offsets, uint64_t n_keys,
                         dbeel_get_result* out,
                         dbeel_get_stats* stats /* may be NULL */);
void dbeel_gpu_get_result_free(dbeel_get_result* r);
/* Frees the reader; a pending compaction is aborted, open scans are ended. */
void dbeel_gpu_reader_close(dbeel_gpu_reader* reader);

/* ---- get_entries: values WITH timestamps, into caller buffers ----
 * LSMTree::get_entry (lsm_tree.rs:674-723) returns EntryValue { data,
 * timestamp }: the replicated read takes max_by_key(timestamp) over the
 * local and the remote answers and only then tests for a tombstone
 * (tasks/db_server.rs:338-363), and a replica answers with
 * ShardResponse::Get(Option<EntryValue>) in bincode
 * (remote_shard_connection.rs:105-113). A stored entry is
 * key_len | key | data_len | data | timestamp, so its bytes from data_len to
 * its end ARE the bincode form of EntryValue; the record of a found key is
 * that contiguous range, copied verbatim.
 *
 * Search: dbeel_gpu_reader_get's, bit for bit — the memtable first, reported
 * at run == n_runs, then the tables newest index first, the first key match
 * winning whatever the timestamps, filters consulted as there. hits[q] has
 * exactly the fields reader_get gives (value_offset / value_len still
 * describe the data bytes inside runs[run].data), and the five counters in
 * stats are those reader_get reports for the same batch.
 *
 * Records: the record of a found key, TOMBSTONES INCLUDED, is the
 * 24 + value_len bytes data_len:u64 | data | timestamp:i128 as stored (the
 * entry's bytes from value_offset - 8 to its end); a tombstone is a 24-byte
 * record; an absent key has an empty range. record_offsets is the exclusive
 * prefix sum of the record sizes over ALL n_keys; hits and record_offsets are
 * always delivered complete, whatever the cap, so the caller can size the
 * next buffer.
 *
 * Paging, stateless: n_done is the largest d with
 * record_offsets[d] <= records_cap; the records of queries [0, n_done) are in
 * records[0 .. records_len); trailing absent queries add no bytes and count
 * as done. With n_done < n_keys the caller calls again with the remaining
 * keys. No device state survives the call, so nothing can go stale under a
 * put, flush or compaction in between; the price is that the next call
 * searches its keys again, about 2 % of a call. If record 0
 * alone exceeds records_cap (n_done == 0 < n_keys; query 0 is then a hit) the
 * call returns DBEEL_ERR_ITEM_TOO_LARGE — the scan's rule; DBEEL_OK with
 * n_done == 0 would make a caller spin — with hits, record_offsets and page
 * (n_done = records_len = 0, needed = its size) still filled.
 *
 * No byte of records at or beyond records_len is written, and no element
 * beyond hits[n_keys-1] or record_offsets[n_keys]. n_keys == 0 succeeds with
 * record_offsets[0] = 0 (when the array is given) and a zeroed page.
 * Zero-length and duplicate keys are legal.
 *
 * Validated on the host before any device call, in this order, each
 * DBEEL_ERR_INVALID_ARG: a NULL reader, buf or page; with n_keys > 0 a NULL
 * keys, key_offsets, hits or record_offsets; NULL records with
 * records_cap > 0; n_keys >= 2^32; key_offsets not ascending. On any failure
 * the reader is as it was.
 *
 * Memory: the engine allocates no host memory for results and registers
 * nothing itself; the copies are hipMemcpyAsync on the reader's stream
 * straight into the caller's buffers, true async DMA when those are
 * registered with dbeel_gpu_pin_host. Device scratch is the reader's own
 * per-batch scratch, shared with reader_get (nothing is retained between
 * calls), the record buffer sized by records_len, not by the cap; none of it
 * counts in table_bytes. One mid-call sync, as reader_get has, fetches the
 * offsets so the host finds n_done by bisection; a final sync ends the call.
 * stats->gather_ms is the offset scan plus the record gather, stats->d2h_ms
 * covers all copies to the caller. */
typedef struct {
    dbeel_lookup_hit* hits;           /* n_keys                              */
    uint64_t*         record_offsets; /* n_keys + 1, exclusive               */
    uint8_t*          records;        /* records_cap bytes; NULL allowed iff
                                         records_cap == 0                    */
    uint64_t          records_cap;
} dbeel_get_buffers;                  /* all caller-owned, never freed here  */

typedef struct {
    uint64_t n_done;        /* leading queries whose records were delivered  */
    uint64_t records_len;   /* == record_offsets[n_done]                     */
    uint64_t records_total; /* == record_offsets[n_keys]                     */
    uint64_t needed;        /* size of record n_done, 0 when n_done==n_keys  */
} dbeel_get_page;

int dbeel_gpu_reader_get_entries(dbeel_gpu_reader* reader,
        const uint8_t* keys, const uint64_t* key_offsets, uint64_t n_keys,
        const dbeel_get_buffers* buf, dbeel_get_page* page,
        dbeel_get_stats* stats /* may be NULL */);

/* ---- get_merged: replicated reads, the newest answer across replicas ----
 * The reference's replicated get (tasks/db_server.rs:338-363) collects the
 * remote replicas' Option<EntryValue> answers, pushes the local one last,
 * takes max_by_key(timestamp) and only then tests for a tombstone. This call
 * does that for a batch on the device: the local reader's answer and up to
 * DBEEL_MERGE_MAX_SOURCES other answers per query go in, only the winners'
 * records come out, in get_entries' record format, caller buffers and paging.
 *
 * Candidates, in order: sources[0] .. sources[n_sources-1], then the local
 * reader LAST, as candidate n_sources (the reference pushes local_value
 * last). A READER candidate answers exactly as get_entries on that reader
 * would (memtable first, reported at run == n_runs, then the tables newest
 * index first, filters consulted as there). An ANSWERS candidate answers
 * query q with records[record_offsets[q] .. record_offsets[q+1]), an empty
 * range meaning absent — the pair a replica's get_entries delivers.
 *
 * Winner: the candidate with the greatest timestamp, the record's last 16
 * bytes as i128 little-endian (a signed high half, then an unsigned low
 * half). Among equal timestamps the HIGHEST candidate index wins — Rust's
 * max_by_key returns the last maximum, so the local answer wins a tie with a
 * remote one. Absent candidates are skipped (flatten). With no candidate
 * holding the key, source = -1 and the record range is empty. A winning
 * tombstone is a 24-byte record with is_tombstone = 1; the client-facing
 * "not found" decision (db_server.rs:361) stays with the caller.
 *
 * stale_mask: bit s is set iff a winner exists and candidate s is absent or
 * strictly older than the winner (an equal timestamp is not stale); without
 * a winner it is 0. It is what read repair needs; no repair is applied here.
 *
 * Records: the winner's record, copied verbatim from its table, memtable or
 * uploaded answer. record_offsets covers all keys; hits and record_offsets
 * are always delivered complete; page (n_done, records_len, records_total,
 * needed) follows get_entries' rule word for word, DBEEL_ERR_ITEM_TOO_LARGE
 * for a first record over the cap included. No byte of records at or beyond
 * records_len is written, and no element beyond hits[n_keys-1] or
 * record_offsets[n_keys]. The call is stateless: the next page is a new call
 * with the remaining keys and every ANSWERS source advanced by the caller
 * (offsets rebased to 0). n_keys == 0 succeeds as in get_entries.
 *
 * n_sources == 0 is legal: record_offsets and records are then byte-identical
 * to get_entries' for the same keys and cap, and every found key has
 * source == 0.
 *
 * Validated on the host before any device call, page and stats zeroed first,
 * in this order, each DBEEL_ERR_INVALID_ARG:
 *   1. a NULL local reader, buf or page;
 *   2. get_entries' own key and buffer checks, in its order;
 *   3. n_sources > DBEEL_MERGE_MAX_SOURCES, or NULL sources with
 *      n_sources > 0;
 *   4. a source of unknown kind;
 *   5. a READER source with a NULL reader, with the local reader itself, or
 *      with a reader on another device;
 *   6. an ANSWERS source with NULL record_offsets, or with NULL records while
 *      record_offsets[n_keys] > 0;
 *   7. an ANSWERS source whose offsets do not start at 0 or do not ascend.
 *
 * Remote bytes are untrusted: an ANSWERS record that is non-empty and shorter
 * than 24 bytes, or whose leading data_len differs from its size - 24, makes
 * the call DBEEL_ERR_CORRUPT. This is found on the device; the message names
 * the source and the query (the lowest of each), and nothing has then been
 * written to any caller buffer. On every failure all readers are as they
 * were.
 *
 * Memory and streams: no host allocation for results, nothing registered by
 * the engine. ANSWERS sources go up with hipMemcpyAsync on the local reader's
 * stream (true async DMA when registered with dbeel_gpu_pin_host). Scratch is
 * reader-owned, grown on demand and reused; none of it counts in table_bytes.
 * A READER source is searched on its own stream into its own scratch, after
 * the keys are up, and that stream is synchronised before the local stream
 * reads its hit records (scan_apply's ordering). The paging rule runs on the
 * device, so one small mid-call read brings back the page, the counters and
 * the error word, and the caller's buffers are written only after that; a
 * final sync ends the call.
 *
 * stats: search_ms sums the search kernels' own times over all reader
 * candidates (sources overlap the local search in wall time); pick_ms is the
 * per-candidate staging plus the pick; gather_ms the offset scan, the page
 * rule and the record gather; d2h_ms every copy to the host. winners counts
 * queries with a winner, tombstones the winners that are tombstones,
 * from_local the winners that are the local answer. */
#define DBEEL_MERGE_ANSWERS 0   /* a replica's get_entries answer, host memory   */
#define DBEEL_MERGE_READER  1   /* another reader on the same device             */
#define DBEEL_MERGE_MAX_SOURCES 15

typedef struct {
    int kind;
    dbeel_gpu_reader* reader;        /* READER                                    */
    const uint64_t* record_offsets;  /* ANSWERS: n_keys + 1, as get_entries gives */
    const uint8_t*  records;         /* ANSWERS: record_offsets[n_keys] bytes     */
} dbeel_merge_source;

typedef struct {
    int32_t  source;        /* winner: 0..n_sources-1, n_sources = local, -1 none */
    uint32_t is_tombstone;  /* winner's data is empty                             */
    uint64_t value_len;     /* winner's data bytes; its record is 24 + value_len  */
    uint64_t stale_mask;    /* bit s: candidate s is absent or older than winner  */
} dbeel_merge_hit;

typedef struct {
    dbeel_merge_hit* hits;            /* n_keys                                   */
    uint64_t*        record_offsets;  /* n_keys + 1, exclusive                    */
    uint8_t*         records;         /* records_cap bytes; NULL iff cap == 0     */
    uint64_t         records_cap;
} dbeel_merge_buffers;                /* all caller-owned, never freed here       */

typedef struct {
    double   h2d_ms, search_ms, pick_ms, gather_ms, d2h_ms;
    uint64_t winners, tombstones, from_local;
} dbeel_merge_stats;

int dbeel_gpu_reader_get_merged(dbeel_gpu_reader* local,
        const uint8_t* keys, const uint64_t* key_offsets, uint64_t n_keys,
        const dbeel_merge_source* sources, size_t n_sources,
        const dbeel_merge_buffers* buf, dbeel_get_page* page,
        dbeel_merge_stats* stats /* may be NULL */);

/* ---- Live reader: the shared sstable list ----
 * The reference's LSMTree keeps one list of open sstables that reads,
 * flushes and compactions share: a flush pushes the new table
 * (lsm_tree.rs:901-915); a compaction partitions out its inputs, pushes
 * the output, sorts and swaps the list while reads in flight finish on the
 * old one (lsm_tree.rs:1113-1145). The reader holds one device table per
 * run (run bytes padded like a job's input, 8 B per entry of prefixes, an
 * optional filter bitmap), so the list can take a flushed run, compact
 * runs it already holds without moving them, and swap in one step. Runs
 * are identified by position in the list — what hit.run reports. Same
 * contract as above: one thread at a time per reader. */
size_t dbeel_gpu_reader_run_count(const dbeel_gpu_reader* reader);

/* Flush: upload ONE run (and its filter, may be NULL) and insert it at
 * position pos in [0, n_runs]; runs at >= pos move up by one. Arguments
 * are validated on the host before any device call (NULL reader/run,
 * pos > n_runs or a reader already at 64 runs: DBEEL_ERR_INVALID_ARG; a
 * bad filter header: DBEEL_ERR_CORRUPT), then the run is uploaded and
 * checked by the open-time device pass, then linked in. On any failure the
 * reader is exactly as it was (same answers, same table_bytes). */
int dbeel_gpu_reader_insert_run(dbeel_gpu_reader* reader, size_t pos,
                                const dbeel_run_view* run,
                                const dbeel_bloom_view* bloom);

/* Compaction of runs the reader already holds, with no input H2D. */
typedef struct {
    dbeel_compact_timings pipeline; /* h2d_ms = 0 by construction        */
    double   adopt_ms;   /* output -> resident table: D2D copy + k_reader_adopt */
    double   d2h_ms;     /* fetch of out / filter bytes, 0 when not asked */
    uint64_t d2h_bytes;
    uint64_t entries_in, entries_out, data_bytes_out;
} dbeel_reader_compact_stats;

/* begin: runs the compaction pipeline over the tables at positions[]
 * (strictly ascending, in range, at least one; n_positions == 1 rewrites
 * one run) in place, copies the output device-to-device into a new
 * right-sized table, builds its prefix array and — when build_bloom — its
 * filter (dbeel_gpu_job_bloom's parameters) in one device pass, and holds
 * that table PENDING: gets keep being answered from the old list until
 * commit. out (NULL = leave the bytes on the device) and bloom_bytes /
 * bloom_len (both NULL, or both set; filled when build_bloom, free with
 * dbeel_gpu_bloom_free) receive exactly the bytes dbeel_gpu_compact and
 * dbeel_gpu_job_bloom give for the same runs. At most one compaction may
 * be pending (a second begin is DBEEL_ERR_INVALID_ARG). On failure
 * (including DBEEL_ERR_OOM) the reader is untouched.
 *
 * commit: removes the input tables and inserts the pending one at out_pos
 * in [0, n_runs - n_positions] — one host-side list edit and a descriptor
 * upload; an empty output stays in the list as an empty run. Nothing
 * pending, or a bad out_pos (the pending table survives it), is
 * DBEEL_ERR_INVALID_ARG.
 *
 * abort: frees the pending table; no-op when nothing is pending. */
int dbeel_gpu_reader_compact_begin(dbeel_gpu_reader* reader,
        const uint32_t* positions, size_t n_positions,
        int keep_tombstones, int build_bloom,
        dbeel_compact_result* out,
        uint8_t** bloom_bytes, uint64_t* bloom_len,
        dbeel_reader_compact_stats* stats /* may be NULL */);
int  dbeel_gpu_reader_compact_commit(dbeel_gpu_reader* reader, size_t out_pos);
void dbeel_gpu_reader_compact_abort(dbeel_gpu_reader* reader);

/* compact_fetch: copies the PENDING table's .data and .index bytes — the
 * bytes compact_begin(out = ...) returns — into the caller's buffers with
 * hipMemcpyAsync on the reader's stream (true async DMA when they are
 * registered with dbeel_gpu_pin_host). No kernel runs and no host memory is
 * allocated: a caller that wants the output in pinned memory uses
 * compact_begin(out = NULL) followed by this call. It can be called any
 * number of times between begin and commit / abort and changes nothing.
 * *data_len / *index_len receive the output's sizes (0 for an empty output),
 * d2h_ms (may be NULL) the copies' time. A NULL argument other than d2h_ms,
 * or nothing pending: DBEEL_ERR_INVALID_ARG (lengths zeroed). A cap too
 * small: DBEEL_ERR_ITEM_TOO_LARGE with *data_len / *index_len set to what is
 * needed, nothing written to the buffers, the pending table kept. */
int  dbeel_gpu_reader_compact_fetch(dbeel_gpu_reader* reader,
        uint8_t* data, uint64_t data_cap, uint8_t* index, uint64_t index_cap,
        uint64_t* data_len, uint64_t* index_len,
        double* d2h_ms /* may be NULL */);

/* ---- Paged migration scan over the resident tables ----
 * dbeel_gpu_scan (below) for runs the reader already holds: the AsyncIter
 * analogue (lsm_tree.rs:141-282) iterating the shared sstable list
 * (`tree.sstables.borrow().clone()`, lsm_tree.rs:177) and feeding migration
 * (tasks/migration.rs:62-131) page by page, straight into caller memory.
 * No run is uploaded, no compaction scratch is allocated, and no entry
 * outside the key range is ever loaded.
 *
 * Filter semantics are exactly dbeel_gpu_scan's: key range
 * [start_key, end_key) with a NULL bound unbounded (a non-NULL zero-length
 * end_key keeps nothing), murmur3_32 seed-0 hash ranges with between_cmp's
 * wrapped case, no dedup, no tombstone filter; yield order = table position
 * ascending, key order within a table. The concatenation of all pages
 * (index offsets rebased) is byte-identical to dbeel_gpu_scan over the same
 * runs and filters, for every choice of caps and max_candidates.
 *
 * begin: bisects each table's resident prefix array for
 * lower_bound(start_key) and lower_bound(end_key) (equal-prefix stretches
 * are settled by bisection with full key compares, never a walk) — one
 * small kernel, one sync, one small D2H. The CANDIDATES are the
 * concatenation over tables of the entries between the two bounds; the
 * scan's cursor is a position in that space. max_candidates bounds how many
 * candidates one page examines (0 = default 2^20; values above 2^31 are
 * clamped to 2^31); per-page device scratch is about 60 B per candidate,
 * belongs to the reader and is reused, like a device page buffer of
 * min(data_cap, resident data bytes); neither counts in table_bytes.
 *
 * next: examines the next min(remaining, max_candidates) candidates.
 * Those passing the hash filter are survivors; the page takes the longest
 * prefix of survivors with summed full_size <= data_cap and count <=
 * index_cap/16, and writes their bytes to data, their 16-B index records
 * (offsets from 0 in every page, like a run file holding the page) to
 * index and, when n_ranges != 0 and range_ids is not NULL, the index of
 * the FIRST range matching each entry's hash (`position`,
 * migration.rs:97-104) to range_ids. The cursor moves to the first
 * survivor not taken, or past the window when all were taken. A page may
 * be short or empty with done = 0: loop until done. If the first survivor
 * is larger than data_cap the call returns DBEEL_ERR_ITEM_TOO_LARGE, sets
 * page->needed to its full_size and leaves the cursor where it was: call
 * again with a larger buffer. Copies are hipMemcpyAsync on the reader's
 * stream (true async DMA when the buffers are registered with
 * dbeel_gpu_pin_host); the engine allocates no host memory for results.
 * Arguments are validated before any device call: a NULL scan, page, data
 * or index, data_cap == 0 or index_cap < 16 is DBEEL_ERR_INVALID_ARG.
 *
 * Liveness: a scan sees the list as dbeel_gpu_reader_get does (a pending
 * compaction is invisible). insert_run, a non-empty write_batch and
 * compact_commit change the list and invalidate every open scan: next then returns DBEEL_ERR_INVALID_ARG
 * ("stale scan") and the caller restarts; compact_begin / compact_abort do
 * not. (Divergence: the reference's iterator keeps its cloned list alive,
 * lsm_tree.rs:175-177; dbeel_gpu_reader_scan_snapshot below does the
 * same.) Any number of scans may be open on a reader, under
 * the same one-thread-per-reader contract; dbeel_gpu_reader_close ends the
 * scans still open, after which their handles must not be used. */
typedef struct dbeel_gpu_reader_scan dbeel_gpu_reader_scan;

typedef struct {
    uint64_t data_len;     /* bytes written to data                         */
    uint64_t n_entries;    /* index records written (16 B each)             */
    uint64_t candidates;   /* in-key-range entries examined by this page    */
    uint64_t needed;       /* on DBEEL_ERR_ITEM_TOO_LARGE: full_size of the
                              entry that did not fit; else 0                */
    int      done;         /* 1 = nothing left after this page              */
    double   flag_ms, emit_ms, copy_ms, d2h_ms; /* HIP events, reader stream:
                              flag kernel (and, under DBEEL_SCAN_NEWEST_ONLY,
                              the shadow pass) | scans + emit | winmap +
                              copy | copies into the caller's buffers      */
} dbeel_scan_page;

int  dbeel_gpu_reader_scan_begin(dbeel_gpu_reader* reader,
        const uint8_t* start_key, size_t start_key_len,
        const uint8_t* end_key,   size_t end_key_len,
        const uint32_t* range_starts, const uint32_t* range_ends,
        size_t n_ranges,
        uint64_t max_candidates /* per page; 0 = default 2^20 */,
        dbeel_gpu_reader_scan** out);
int  dbeel_gpu_reader_scan_next(dbeel_gpu_reader_scan* scan,
        uint8_t* data, size_t data_cap,
        uint8_t* index, size_t index_cap,        /* bytes */
        uint32_t* range_ids /* NULL or index_cap/16 slots */,
        dbeel_scan_page* page);
/* Frees the scan; NULL is a no-op. */
void dbeel_gpu_reader_scan_end(dbeel_gpu_reader_scan* scan);

/* ---- Snapshot scans: the memtable as last segment, no stale scans,
 * shadowed versions dropped on the device ----
 * The reference's AsyncIter clones the sstable list — "the sstable files we
 * operate on will not be deleted until this object is dropped"
 * (lsm_tree.rs:175-177) — and yields the sstables and then the memtable
 * (lsm_tree.rs:155-173, 279). scan_snapshot opens a scan that does both;
 * pages are drawn with dbeel_gpu_reader_scan_next and the scan is ended with
 * dbeel_gpu_reader_scan_end, and dbeel_gpu_reader_scan_begin's filters, hash
 * function, between_cmp wrapped case, range_ids, ITEM_TOO_LARGE protocol and
 * page shape apply unchanged.
 *
 * Segments: the tables at positions 0 .. n_runs-1 as the list stands at the
 * call (a pending compaction output is invisible, as for gets) and, with
 * DBEEL_SCAN_MEMTABLE and a non-empty memtable, the memtable as it stands at
 * the call as the LAST segment, its key-range bounds bisected on its own
 * prefix array. Yield order: segment ascending, key order within a segment.
 * With flags == 0 the pages concatenated are byte-identical to the old
 * scan's; with an empty memtable DBEEL_SCAN_MEMTABLE changes nothing. A page
 * never mixes table entries with memtable entries (64 tables plus the
 * memtable are 65 segments, one more than a descriptor holds): the page that
 * exhausts the tables may be short, the next one starts the memtable
 * segment, and done is set only when both are exhausted. The concatenation
 * stays independent of caps and max_candidates.
 *
 * Snapshot: nothing done to the reader afterwards — insert_run, write_batch,
 * compact_begin / commit / abort, put, memtable_flush, memtable_clear —
 * changes what the scan yields or makes it stale; the remaining pages are
 * those that would have followed had they been drawn at once.
 * dbeel_gpu_reader_close still ends every open scan.
 *
 * Ownership: a table's device buffers are reference-counted — one reference
 * for the list, one per snapshot scan; compact_commit drops the list's and
 * the last holder frees. The memtable buffer a snapshot reads is held the
 * same way: a put about to write into a held buffer of the ping-pong pair
 * hands it over to its holders and takes a fresh one for the pair. The call
 * copies nothing whose size depends on the memtable. table_bytes counts the
 * list (plus pending) and memtable_info.reserved_bytes the pair, as before;
 * dbeel_gpu_reader_held_bytes counts the device bytes that belong to neither
 * any more and live only because a scan holds them, each buffer once: 0
 * right after the call, 0 again when the holding scans have ended. A failed
 * call leaves the reader, its memtable, its scans and all three counts as
 * they were.
 *
 * DBEEL_SCAN_NEWEST_ONLY: an entry of segment s is dropped when a segment
 * t > s OF THE SNAPSHOT holds a byte-equal key (a tombstone shadows like any
 * entry and is itself emitted when it is the last version; without
 * DBEEL_SCAN_MEMTABLE the memtable neither appears nor shadows). The
 * receiver applies entries in arrival order through a set() that replaces
 * whatever the timestamps are (rbtree_arena/src/lib.rs:497-511,
 * tasks/migration.rs:62-131), so its final state is unchanged. The result
 * equals filtering first and then keeping, per key, the entry of the highest
 * segment. The shadowing entry is looked for in the whole later segment,
 * wherever the page windows fall. A dropped entry counts in
 * page->candidates and in info.shadowed. flag_ms of a page INCLUDES the
 * shadow pass. The pass has two variants with the same result, chosen by
 * DBEEL_SCAN_SHADOW in the environment, read on every next: "full" (the
 * default) bisects each whole later segment per candidate; "narrow"
 * bisects, per block of 256 consecutive candidates, only the slice of each
 * later segment the block's keys can fall into. The two measured level on
 * cfg3, so the plainer one is the default.
 *
 * Validated on the host before any device call, in this order: flag bits
 * other than the two defined (DBEEL_ERR_INVALID_ARG, the message names the
 * flags); then dbeel_gpu_reader_scan_begin's checks in its order.
 *
 * scan_info works on either kind of scan; one opened by scan_begin reports
 * n_tables, table_candidates and zeros elsewhere. A NULL scan or info is
 * DBEEL_ERR_INVALID_ARG. held_bytes(NULL) is 0. */
#define DBEEL_SCAN_MEMTABLE     1u  /* the memtable is the last segment      */
#define DBEEL_SCAN_NEWEST_ONLY  2u  /* drop entries shadowed by a later one  */

typedef struct {
    uint32_t n_tables;            /* tables in the snapshot                       */
    uint32_t has_memtable;        /* 1 = a non-empty memtable segment is included */
    uint64_t table_candidates;    /* in-key-range entries, tables                 */
    uint64_t memtable_candidates; /* in-key-range entries, memtable segment       */
    uint64_t shadowed;            /* entries dropped by NEWEST_ONLY so far        */
} dbeel_scan_snapshot_info;

int dbeel_gpu_reader_scan_snapshot(dbeel_gpu_reader* reader,
        const uint8_t* start_key, size_t start_key_len,
        const uint8_t* end_key,   size_t end_key_len,
        const uint32_t* range_starts, const uint32_t* range_ends,
        size_t n_ranges,
        uint64_t max_candidates /* per page; 0 = default 2^20 */,
        uint32_t flags, dbeel_gpu_reader_scan** out);
int dbeel_gpu_reader_scan_info(const dbeel_gpu_reader_scan* scan,
                               dbeel_scan_snapshot_info* info);
uint64_t dbeel_gpu_reader_held_bytes(const dbeel_gpu_reader* reader);

/* ---- Run encoder (the memtable-flush path) ----
 * Encodes an already-sorted (key, value, timestamp) stream into a run:
 * the same entry layout + 16-byte index records flush_memtable_to_disk /
 * EntryWriter produce (lsm_tree.rs:925-946, entry_writer.rs:71-98).
 * keys/values: concatenated byte blobs with n+1 exclusive offsets;
 * timestamps: n x 16-byte little-endian i128. Outputs are engine-allocated
 * (dbeel_gpu_result_free). Oversized entries (full_size > u32::MAX) return
 * DBEEL_ERR_ITEM_TOO_LARGE (error.rs:60-61). */
int dbeel_gpu_encode_run(uint64_t n_entries, const uint8_t* keys,
                         const uint64_t* key_offsets, const uint8_t* values,
                         const uint64_t* value_offsets,
                         const uint8_t* timestamps, int device,
                         dbeel_compact_result* out);

/* ---- Write batch (the memtable and its flush, on the device) ----
 * The reference's memtable is a RedBlackTree<Vec<u8>, EntryValue> whose set
 * replaces the value of an equal key WHATEVER the timestamps are
 * (rbtree_arena/src/lib.rs:497-511); flush iterates it in key order into
 * EntryWriter (lsm_tree.rs:882-889, 925-946) and pushes the table onto the
 * end of the sstable list with no bloom (lsm_tree.rs:901-915); an empty
 * memtable flushes nothing (lsm_tree.rs:850-852).
 *
 * Input: n_writes writes in ARRIVAL order (array order), unsorted, keys may
 * repeat — the arrays of dbeel_gpu_encode_run; an empty value is a
 * tombstone. Output run: one entry per distinct key, keys ascending in
 * byte-lexicographic order (a proper prefix first, the empty key legal),
 * each with the value and timestamp of its LAST arrival, even when an
 * earlier arrival has a larger timestamp; tombstones are kept. The bytes
 * are what dbeel_gpu_encode_run returns for that sorted, deduplicated
 * stream.
 *
 * reader_write_batch sorts, deduplicates and encodes the batch straight
 * into a new right-sized resident table and inserts it at pos in
 * [0, n_runs] exactly as dbeel_gpu_reader_insert_run would (pos == n_runs
 * is the reference's push: gets see it first; open scans go stale; a
 * pending compaction's positions shift). out (NULL = leave the bytes on the
 * device) receives the run for the caller to persist; with build_bloom the
 * table gets a filter with dbeel_gpu_job_bloom's parameters, and
 * bloom_bytes / bloom_len (both NULL, or both set; free with
 * dbeel_gpu_bloom_free) its "DBLM" file — the bytes compact_begin({pos},
 * keep_tombstones = 1, build_bloom = 1) returns for the table afterwards.
 * All device work runs on the reader's stream; uploads are true async DMA
 * when the arrays are registered with dbeel_gpu_pin_host. Staging and sort
 * scratch belong to the call.
 *
 * Validated on the host before any device call, in this order: NULL reader,
 * or a NULL array with n_writes != 0; pos > n_runs; a mismatched bloom
 * pair; n_writes >= 2^31; a descending offset; a reader at 64 runs with
 * n_writes != 0 (all DBEEL_ERR_INVALID_ARG); a write with
 * 32 + klen + vlen > u32::MAX (DBEEL_ERR_ITEM_TOO_LARGE). n_writes == 0 is
 * a successful no-op: no table, no generation change, zeroed outputs. On
 * any failure the reader answers as before and holds the same table_bytes.
 *
 * The order stage has two paths with the same result, chosen by
 * DBEEL_BATCH_ORDER in the environment, read on every call: "merge" (the
 * default: it measured faster on most shapes) is one merge
 * sort over all writes by (8-byte key prefix, key, arrival); "radix" is a
 * stable radix sort on (prefix, arrival) followed by a merge sort of only
 * the writes whose prefix equals another's (stats.prefix_tied counts them
 * on both paths).
 *
 * flush_batch is the same pipeline with no reader: bytes only. */
typedef struct {
    double   h2d_ms, order_ms, encode_ms, adopt_ms, d2h_ms; /* HIP events on
                 the reader's stream: upload | prefixes + order | survivor
                 flags, scans, table allocation, encode | k_reader_adopt |
                 fetch of out / filter bytes, 0 when not asked */
    uint64_t writes_in, entries_out, data_bytes_out;
    uint64_t prefix_tied;  /* writes whose 8-byte prefix equals another write's */
    uint64_t d2h_bytes;
} dbeel_write_batch_stats;

int dbeel_gpu_reader_write_batch(dbeel_gpu_reader* reader, size_t pos,
        uint64_t n_writes, const uint8_t* keys, const uint64_t* key_offsets,
        const uint8_t* values, const uint64_t* value_offsets,
        const uint8_t* timestamps, int build_bloom,
        dbeel_compact_result* out /* NULL = leave on device */,
        uint8_t** bloom_bytes, uint64_t* bloom_len /* both or neither */,
        dbeel_write_batch_stats* stats /* may be NULL */);

int dbeel_gpu_flush_batch(uint64_t n_writes, const uint8_t* keys,
        const uint64_t* key_offsets, const uint8_t* values,
        const uint64_t* value_offsets, const uint8_t* timestamps,
        int device, dbeel_compact_result* out);

/* ---- Resident memtable: puts visible to gets, flushed as one run ----
 * LSMTree::get_entry's first step (the active memtable, then the sstables
 * newest-first, lsm_tree.rs:674-723) and the flush that ends it
 * (lsm_tree.rs:850-915), with the memtable resident in HBM and owned by the
 * reader.
 *
 * State: the memtable is ONE sorted run with unique keys in the resident
 * table layout (16 B pad | data | index | 16 B pad, plus the dense 8-byte
 * prefix array). It is not in the table list. Invariant: after puts
 * W1 ... Wk since the last flush or clear, its data and index bytes are
 * exactly dbeel_gpu_flush_batch(W1 || ... || Wk): one entry per distinct
 * key, keys ascending bytewise, each with the value and timestamp of its
 * LAST arrival whatever the timestamps are (the rbtree's set(),
 * rbtree_arena/src/lib.rs:497-511), tombstones kept. An empty memtable
 * changes nothing anywhere: every other call behaves, and reports
 * table_bytes, exactly as without one.
 *
 * Get: dbeel_gpu_reader_get consults the memtable first
 * (lsm_tree.rs:676-685). A key found there is a hit with
 * run == dbeel_gpu_reader_run_count(reader) — the position the flush will
 * give it; value_offset indexes the memtable's data bytes and is valid
 * until the next put, flush or clear; is_tombstone and value_len work as for
 * a table and the value bytes are packed into values like any other hit. A
 * get just before memtable_flush and the same get just after return
 * identical hits, offsets and value bytes. In dbeel_get_stats a non-empty
 * memtable counts as one visit to an unfiltered run (searches).
 *
 * Liveness: a put does not edit the table list and bumps no generation, so
 * open scans stay valid. Scans do NOT see the memtable (documented
 * divergence from lsm_tree.rs:155-173: the caller flushes before
 * migrating, or opens the scan with dbeel_gpu_reader_scan_snapshot and
 * DBEEL_SCAN_MEMTABLE). A non-empty flush is a list edit at the end: open scans go
 * stale, a pending compaction's positions do not move. A reader at 64
 * tables still takes puts and answers from them (hit.run == 64);
 * memtable_flush on it is DBEEL_ERR_INVALID_ARG and keeps the memtable. On
 * any failure of any call below, the reader, its memtable and its answers
 * are exactly as before.
 *
 * put: the arrays of dbeel_gpu_reader_write_batch, in arrival order. The
 * batch is ordered and deduplicated by the write batch's own stages
 * (DBEEL_BATCH_ORDER applies), then merged into the memtable on the device,
 * the batch winning equal keys. Validated on the host before any device
 * call, in this order: NULL reader, or a NULL array with n_writes != 0;
 * n_writes >= 2^31; a descending offset; memtable entries + n_writes >=
 * 2^31 (all DBEEL_ERR_INVALID_ARG); a write with 32 + klen + vlen >
 * u32::MAX (DBEEL_ERR_ITEM_TOO_LARGE). n_writes == 0 is a successful no-op.
 *
 * Storage: a ping-pong pair of buffers that grows geometrically; a put
 * writes the new memtable into the other buffer and swaps on success, and
 * allocates only when it outgrows the pair. The pair is kept across flush
 * and clear, freed by dbeel_gpu_reader_close, reported as
 * memtable_info.reserved_bytes and not part of table_bytes. Staging and
 * merge scratch belong to the call.
 *
 * fetch: copies the memtable's run bytes to the host (engine-allocated,
 * dbeel_gpu_result_free) and changes nothing — for a caller that persists
 * before it links. An empty memtable gives zeroed outputs and success.
 *
 * flush: an empty memtable is a no-op — no table, no generation change,
 * zeroed outputs (lsm_tree.rs:850-852). Otherwise the memtable becomes a
 * right-sized table at position n_runs (device-to-device copy; prefixes
 * and, when build_bloom, a filter with dbeel_gpu_job_bloom's parameters in
 * one pass), after which table_bytes equals a fresh reader's over the same
 * runs, and the memtable is empty with its storage kept. out (NULL = leave
 * the bytes on the device) and bloom_bytes / bloom_len (both NULL, or both
 * set; free with dbeel_gpu_bloom_free) are what
 * dbeel_gpu_reader_write_batch returns for the concatenated arrivals.
 *
 * clear: drops the contents, keeps the storage. */
typedef struct {
    double   h2d_ms, order_ms, merge_ms;  /* HIP events, reader stream: upload |
                 prefixes + order + batch encode | rank, scans, emit, copy, prefixes */
    uint64_t writes_in, batch_entries;    /* distinct keys in this batch          */
    uint64_t replaced;                    /* memtable entries this batch overwrote */
    uint64_t entries, data_bytes;         /* memtable after the put               */
    uint64_t prefix_tied;                 /* as dbeel_write_batch_stats           */
} dbeel_memtable_put_stats;

typedef struct { uint64_t entries, data_bytes, reserved_bytes, puts; } dbeel_memtable_info;

int  dbeel_gpu_reader_put(dbeel_gpu_reader* reader, uint64_t n_writes,
        const uint8_t* keys, const uint64_t* key_offsets,
        const uint8_t* values, const uint64_t* value_offsets,
        const uint8_t* timestamps,
        dbeel_memtable_put_stats* stats /* may be NULL */);
int  dbeel_gpu_reader_memtable_info(const dbeel_gpu_reader* reader,
        dbeel_memtable_info* info);
int  dbeel_gpu_reader_memtable_fetch(dbeel_gpu_reader* reader,
        dbeel_compact_result* out);
int  dbeel_gpu_reader_memtable_flush(dbeel_gpu_reader* reader, int build_bloom,
        dbeel_compact_result* out /* NULL = leave on device */,
        uint8_t** bloom_bytes, uint64_t* bloom_len /* both or neither */);
void dbeel_gpu_reader_memtable_clear(dbeel_gpu_reader* reader);

/* ---- Scan pages applied as puts or deletes (migration inside HBM) ----
 * The receiving end of the migration loop (tasks/migration.rs:62-131): per
 * iterated entry the reference picks the first matching hash range, looks up
 * that range's action and either sends Set(key, data, timestamp) to another
 * shard — whose set_with_timestamp (shards.rs:768) replaces whatever the
 * timestamps are — or calls tree.delete(key) on its own tree.
 *
 * put_entries: takes a page exactly as dbeel_gpu_reader_scan_next writes it:
 * n_entries entries in the run entry format in data (data_len bytes), their
 * 16-byte index records in index with offsets from 0, monotone and
 * non-overlapping, in arrival order (= index order); keys unsorted and
 * possibly repeated. Entry i is selected when range_ids == NULL or
 * take[range_ids[i]] != 0. Under DBEEL_APPLY_PUT the memtable afterwards is
 * the memtable after dbeel_gpu_reader_put of the selected entries, decoded
 * and in page order (last arrival wins whatever the timestamps are,
 * tombstones kept, bytes equal to dbeel_gpu_flush_batch of all arrivals
 * since the last flush); a survivor is the verbatim bytes of its page entry.
 * Under DBEEL_APPLY_DELETE it is the memtable after a put of (key, empty
 * value, delete_ts) for every selected entry — tree.delete(key) per yielded
 * entry. Documented divergence: the whole call carries ONE timestamp, where
 * the reference reads the clock per delete. Gets, flush, fetch, snapshot
 * scans and holds behave as after a put; DBEEL_BATCH_ORDER applies.
 *
 * Validated on the host before any device call, in this order: NULL reader;
 * NULL data or index with n_entries != 0; a mode other than the two
 * defined; DELETE without delete_ts; range_ids without take or with
 * n_take == 0; n_entries >= 2^31; memtable entries + n_entries >= 2^31 (all
 * DBEEL_ERR_INVALID_ARG). n_entries == 0 is a successful no-op.
 *
 * Validated on the device (one implementation serves host pages and pages
 * already resident, see scan_apply): every entry, selected or not, passes
 * the run loader's bounds check and consistency check (offset and sizes
 * inside data_len, the bincode length fields agreeing with the index
 * record, the successor's offset not overlapping) before anything is read
 * through it; a failing entry is DBEEL_ERR_CORRUPT. A selected entry with
 * range_ids[i] >= n_take is DBEEL_ERR_INVALID_ARG. On these and on every
 * other failure the reader, its memtable and its answers are exactly as
 * before. A call that selects nothing is a successful no-op:
 * memtable_info.puts does not move.
 *
 * Stats: as dbeel_memtable_put_stats; entries_in = n_entries, selected =
 * entries the mask let through, h2d_ms = 0 for a device-resident page.
 *
 * scan_apply: draws the next page exactly as dbeel_gpu_reader_scan_next
 * would with data_cap = page_bytes and index_cap = 16 * page_entries
 * (cursor rule, done, the ITEM_TOO_LARGE protocol with page->needed,
 * stale-scan refusal, snapshot behaviour and the shadow pass are the same),
 * leaves it in the reader's device page buffer and applies it there:
 * actions[id] says what happens to the entries whose first matching range
 * is id; n_actions must equal the scan's n_ranges, and a scan without hash
 * ranges takes n_actions == 1 with every entry under actions[0]. SKIP drops
 * the entry (a caller with a remote destination scans those ranges with
 * scan_next); PUT goes to dst's memtable; DELETE puts a tombstone carrying
 * delete_ts into dst's memtable — normally the scan's own reader, as in the
 * reference. Entries are grouped by distinct (kind, dst), in ascending order
 * of each group's first range id; each group is one device run of
 * put_entries over the same resident page with that group's take mask.
 * page->d2h_ms is 0. dst may be the scan's own reader: puts bump no
 * generation and snapshot scans hold their buffers.
 *
 * Refused before any device call (DBEEL_ERR_INVALID_ARG, the cursor and
 * everything else untouched), in this order: NULL scan or page (page and
 * stats are zeroed first); NULL actions; n_actions mismatch; an unknown
 * kind; PUT or DELETE with a NULL dst; a dst on another device than the
 * scan's reader; DELETE without delete_ts; page_bytes == 0 or
 * page_entries == 0; a stale scan.
 *
 * Failure: the cursor advances only after every group succeeded. If group g
 * fails, the groups before it stay applied and the cursor stays; calling
 * again re-applies the same page, which for a destination that took no
 * other writes in between reaches the same state because a set replaces —
 * the reference's re-send.
 *
 * Streams: the page is finished on the scan reader's stream, which is
 * synchronised before any destination's stream reads it; each destination
 * is synchronised before the call returns, so the next page overwrites a
 * buffer nobody reads. */
#define DBEEL_APPLY_SKIP   0
#define DBEEL_APPLY_PUT    1
#define DBEEL_APPLY_DELETE 2

typedef struct {
    double   h2d_ms, order_ms, merge_ms;  /* as dbeel_memtable_put_stats; order_ms
                 covers stage + order + encode                                   */
    uint64_t entries_in, selected;        /* page entries | those the mask took   */
    uint64_t batch_entries, replaced;     /* as dbeel_memtable_put_stats          */
    uint64_t entries, data_bytes;         /* memtable after the call              */
    uint64_t prefix_tied;
} dbeel_put_entries_stats;

int  dbeel_gpu_reader_put_entries(dbeel_gpu_reader* reader,
        const uint8_t* data, uint64_t data_len,
        const uint8_t* index, uint64_t n_entries,     /* 16-B records */
        const uint32_t* range_ids /* NULL = every entry selected */,
        const uint8_t* take, uint32_t n_take,         /* take[id] != 0 selects */
        int mode /* DBEEL_APPLY_PUT | DBEEL_APPLY_DELETE */,
        const uint8_t* delete_ts /* 16 B, i128 LE; DELETE only */,
        dbeel_put_entries_stats* stats /* may be NULL */);

typedef struct { int kind; dbeel_gpu_reader* dst; } dbeel_apply_action;

typedef struct {
    double   apply_ms;                    /* wall: page drawn -> last group merged */
    uint64_t put_entries, delete_entries; /* page entries under each kind         */
    uint64_t skipped;                     /* page entries under SKIP              */
    uint64_t groups;                      /* device runs of put_entries           */
} dbeel_scan_apply_stats;

int  dbeel_gpu_reader_scan_apply(dbeel_gpu_reader_scan* scan,
        const dbeel_apply_action* actions, size_t n_actions,
        const uint8_t* delete_ts /* needed iff some kind is DELETE */,
        uint64_t page_bytes, uint64_t page_entries,
        dbeel_scan_page* page, dbeel_scan_apply_stats* stats /* may be NULL */);

/* ---- Resident-job API (benchmarking / repeated compactions) ----
 * Uploads the runs to `device` once; each run executes the device pipeline
 * with inputs already resident in HBM (what BASELINE's MB/s is quoted on)
 * and leaves outputs on the device. */
typedef struct dbeel_gpu_job dbeel_gpu_job;

int dbeel_gpu_job_create(const dbeel_run_view* runs, size_t n_runs,
                         int device, dbeel_gpu_job** out_job);
/* Batched INDEPENDENT jobs in one launch set (one dbeel shard each —
 * BASELINE configs[3]'s many-jobs-per-GPU shape): runs[] holds every
 * job's runs back to back, runs_per_job[] their counts (each >= 1,
 * summing to n_runs). Jobs never interact: ranks, crossrank slots and
 * newest-wins flags are job-local, and a key present in two jobs
 * survives in both. Outputs land concatenated in job order;
 * dbeel_gpu_job_fetch_job slices job `job_idx`'s result back out with
 * index offsets rebased to its own run file. job_run/job_ingest/
 * job_fetch work on batched jobs unchanged (fetch returns the
 * concatenation). */
int dbeel_gpu_job_create_batched(const dbeel_run_view* runs, size_t n_runs,
                                 const uint32_t* runs_per_job,
                                 size_t n_jobs, int device,
                                 dbeel_gpu_job** out_job);
int dbeel_gpu_job_fetch_job(dbeel_gpu_job* job, size_t job_idx,
                            dbeel_compact_result* out);
/* Runs the pipeline; fills t (may be NULL) and the output sizes. */
int dbeel_gpu_job_run(dbeel_gpu_job* job, int keep_tombstones,
                      uint64_t* out_data_len, uint64_t* out_entries,
                      dbeel_compact_timings* t);
/* Copies the last run's outputs to host (engine-allocated). */
int dbeel_gpu_job_fetch(dbeel_gpu_job* job, dbeel_compact_result* out);
/* Builds the behavioral "DBLM" bloom over the last run's surviving keys
 * on the device (the Bloom::set-per-written-key step,
 * lsm_tree.rs:1049-1051; format in include/dbeel_lsm.h). Engine-allocated;
 * free with dbeel_gpu_bloom_free. */
int dbeel_gpu_job_bloom(dbeel_gpu_job* job, uint8_t** out_bytes,
                        uint64_t* out_len);
void dbeel_gpu_bloom_free(uint8_t* p);
void dbeel_gpu_job_destroy(dbeel_gpu_job* job);

/* ---- Streamed pinned ingest (north_star: "input SSTable runs are
 * pinned in host DRAM and streamed via hipMemcpyAsync with compute
 * overlap") ----
 *
 * dbeel_gpu_pin_host / unpin_host: page-lock a caller buffer
 * (hipHostRegister) so streamed copies run as true async DMA. A
 * production engine pins its run staging buffers once; pin before the
 * hot loop, not inside it.
 *
 * dbeel_gpu_job_ingest: re-uploads fresh run contents into an EXISTING
 * job's resident input slab, streaming each run's data in
 * entry-boundary-aligned chunks (default 64 MiB, env
 * DBEEL_STREAM_CHUNK_MB) on a dedicated copy stream while k_prepare
 * runs on already-arrived chunks on the compute stream — the
 * copy-engine/compute overlap the reference gets from its 16-deep
 * read-ahead DmaStreamReaders (lsm_tree.rs:974-993). Run shapes
 * (data_len/index_len per run) must match the job's. After a successful
 * ingest the job's prepare stage is already done: the next
 * dbeel_gpu_job_run skips it (the work happened, hidden behind the
 * PCIe transfer). stats (may be NULL) reports the wall ingest time and
 * how much prepare time was hidden. */
typedef struct {
    double ingest_ms;   /* wall: first copy enqueued -> all chunks +
                           prepare complete */
    double copy_ms;     /* pure H2D transfer time (copy stream span) */
    double prep_ms;     /* prepare kernel time, overlapped with copies */
    uint64_t bytes;     /* total bytes ingested (data + index) */
    uint64_t chunks;
} dbeel_ingest_stats;

int dbeel_gpu_pin_host(const void* ptr, size_t len);
int dbeel_gpu_unpin_host(const void* ptr);

/* The grid every launch outside the copy and co-rank kernels uses for
 * work_items items (or work_items * 64 lanes for a wave-per-item kernel) in
 * blocks of `block` threads: ceil(work_items / block), at least 1, capped;
 * past the cap the kernels cover the rest with a grid-stride loop. Pure host
 * arithmetic, no device call; block == 0 returns 0. Exported so that tests
 * can size their inputs past the cap whatever its value. */
uint32_t dbeel_gpu_grid_for(uint64_t work_items, uint32_t block);
int dbeel_gpu_job_ingest(dbeel_gpu_job* job, const dbeel_run_view* runs,
                         size_t n_runs, dbeel_ingest_stats* stats);

/* ---- Batched migration / iteration scan ----
 * GPU analogue of AsyncIter (lsm_tree.rs:141-282) feeding migration
 * (tasks/migration.rs:62-131): yields entries in the reference's yield
 * order — sstables ascending by index, entries in key order within each
 * (IterState walks index 0 upward, lsm_tree.rs:210-276) — with NO dedup
 * and NO tombstone filtering (the reference iterator yields every entry;
 * migration re-sends duplicates and resolves by timestamp at the
 * destination). Filters, combinable (entry kept iff it passes all):
 *   - key range [start_key, end_key), either bound NULL = unbounded;
 *   - murmur3_32(key, seed 0) hash ranges with wraparound semantics
 *     (hash_bytes shards.rs:99-101, murmur3 crate v0.5.2 restated;
 *     between_cmp tasks/migration.rs:54-60: start <= end means
 *     [start, end), end < start wraps to hash >= start || hash < end...
 *     precisely: kept iff hash < start || hash >= end when end < start).
 * Output = packed entries verbatim + rebuilt 16-B index records, like a
 * run file holding exactly the yielded entries. */
int dbeel_gpu_scan(const dbeel_run_view* runs, size_t n_runs,
                   const uint8_t* start_key, size_t start_key_len,
                   const uint8_t* end_key, size_t end_key_len,
                   const uint32_t* range_starts, const uint32_t* range_ends,
                   size_t n_ranges, int device, dbeel_compact_result* out);

/* ---- Sliced compaction (runs larger than HBM) ----
 * Splits the key space into slices that fit max_resident_bytes of input,
 * compacts each slice independently (equal keys never split: slice
 * boundaries are strict key pivots) and concatenates the outputs —
 * byte-identical to one whole-job compaction of the same runs.
 * max_resident_bytes = 0 picks a default from free device memory. */
int dbeel_gpu_compact_sliced(const dbeel_run_view* runs, size_t n_runs,
                             int keep_tombstones, int device,
                             uint64_t max_resident_bytes,
                             dbeel_compact_result* out);

/* ---- Compaction into caller buffers: pipelined slices, bloom across
 * slices ----
 *
 * job_fetch_into: dbeel_gpu_job_fetch into caller memory. The last run's
 * .data and .index bytes are copied with hipMemcpyAsync on the job's stream
 * (true async DMA when the buffers are registered with dbeel_gpu_pin_host);
 * no host memory is allocated. Every index record's offset leaves with
 * index_base added — the place of this output inside a larger file. The
 * addition runs ON THE DEVICE and INTO SCRATCH: with index_base != 0 the
 * records are copied device-to-device into a buffer of the job that is dead
 * between runs (the rank records) and rebased there by k_index_rebase, so
 * the job's own output index is never modified and a later job_fetch,
 * job_fetch_job, job_bloom or another fetch_into sees the un-rebased result.
 * *data_len / *index_len receive the output's sizes, d2h_ms (may be NULL)
 * the copies' time. A NULL argument other than d2h_ms, or a job without a
 * result: DBEEL_ERR_INVALID_ARG (lengths zeroed). A cap too small:
 * DBEEL_ERR_ITEM_TOO_LARGE with *data_len / *index_len set to what is
 * needed and nothing written to the buffers. */
int dbeel_gpu_job_fetch_into(dbeel_gpu_job* job,
        uint8_t* data, uint64_t data_cap, uint8_t* index, uint64_t index_cap,
        uint64_t index_base, uint64_t* data_len, uint64_t* index_len,
        double* d2h_ms /* may be NULL */);

/* compact_into: dbeel_gpu_compact with the output written into the caller's
 * data / index buffers — byte-identical to dbeel_gpu_compact for the same
 * runs, whatever the slice count. The key space is cut into S slices at
 * strict key pivots (dbeel_gpu_compact_sliced's: evenly spaced keys of the
 * largest run, so an equal-key group never splits); each slice is an
 * ordinary job, and slice i's output travels to the host while slice i+1's
 * input travels to the device:
 *
 *   create job i (upload) -> run -> start its fetch at the running output
 *   offsets -> WITHOUT waiting, create + run job i+1 -> wait for job i's
 *   copies, destroy it -> start job i+1's fetch -> ...
 *
 * Two jobs are alive at once. A slice with no input entries is skipped; a
 * slice with no survivors moves no offsets. One slice is a legal outcome
 * and goes through the same code.
 *
 * S: n_slices > 0 asks for that many. n_slices == 0 uses
 * dbeel_gpu_compact_sliced's budget rule, S = ceil(input bytes / budget),
 * budget = max_resident_bytes, or with max_resident_bytes == 0 a SIXTH of
 * the device's free memory (half of compact_sliced's third, because two jobs
 * are alive). Either way S is capped so that the largest run has at least
 * two entries per slice (S <= max_count / 2, at least 1).
 *
 * No per-entry host loop: a slice's input index records are uploaded as
 * they are and a device pass (k_index_rebase) subtracts the slice's first
 * data offset; the output records get the running output offset added by
 * the same kernel (see job_fetch_into). A record of a slice that points
 * below the slice's first byte wraps to a huge offset and is refused by the
 * entry loader's bounds test like any other corrupt record
 * (DBEEL_ERR_CORRUPT from the slice's run).
 *
 * Caps: a caller that sizes data at the sum of the runs' data_len and index
 * at the sum of their index_len can never be refused (survivors are copied
 * verbatim). When the output does not fit, the call keeps running the
 * remaining slices without copying and returns DBEEL_ERR_ITEM_TOO_LARGE with
 * the exact sizes needed in *result; bytes inside the caps are then
 * unspecified, bytes past the caps are never touched, and no filter is
 * returned.
 *
 * Bloom: with want_bloom != 0 (bloom_bytes and bloom_len both required;
 * free with dbeel_gpu_bloom_free) the "DBLM" filter over all surviving keys
 * is built across slices: per slice k_bloom_hash appends the two 64-bit
 * hashes of every survivor to a device array owned by the call (16 B per
 * survivor, grown geometrically), and once the total survivor count — and
 * with it n_bits — is known, k_bloom_fill sets the bits. The bytes equal
 * dbeel_gpu_job_bloom's on the whole job. With want_bloom == 0 neither
 * kernel is launched.
 *
 * Validated on the host before any device call, in this order: NULL result
 * (then *result, *stats and the bloom outputs are zeroed), NULL data or
 * index, want_bloom with a NULL bloom_bytes or bloom_len, NULL runs /
 * n_runs == 0 / n_runs > 64 (DBEEL_ERR_INVALID_ARG); device < 0
 * (DBEEL_ERR_INVALID_ARG); a bad run view (dbeel_gpu_job_create's codes);
 * then, when S > 1, a corrupt index record met during pivot selection
 * (DBEEL_ERR_CORRUPT). With n_slices == 0 and max_resident_bytes == 0 the
 * free-memory query precedes pivot selection.
 *
 * stats (may be NULL), all from HIP events and host clocks — nothing is
 * counted on the device: slices = jobs actually run; bytes_in = input bytes
 * uploaded; bytes_out = data + index bytes of the output; h2d_ms /
 * kernel_ms / d2h_ms = sums over slices; wall_ms = the whole call;
 * overlap_ms = summed time during which a slice's upload and the previous
 * slice's fetch were both in flight. */
typedef struct {
    uint64_t data_len;        /* output .data bytes (needed, when refused) */
    uint64_t index_len;       /* output .index bytes (needed, when refused) */
    uint64_t entries_written;
} dbeel_compact_into_result;

typedef struct {
    uint64_t slices, bytes_in, bytes_out;
    double   h2d_ms, kernel_ms, d2h_ms, wall_ms, overlap_ms;
} dbeel_compact_into_stats;

int dbeel_gpu_compact_into(const dbeel_run_view* runs, size_t n_runs,
        int keep_tombstones, int device, uint64_t max_resident_bytes,
        uint32_t n_slices,
        uint8_t* data, uint64_t data_cap, uint8_t* index, uint64_t index_cap,
        int want_bloom, uint8_t** bloom_bytes, uint64_t* bloom_len,
        dbeel_compact_into_result* result,
        dbeel_compact_into_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* DBEEL_GPU_H */
