/* dbeel_lsm.h — file-level host layer over the compaction engine.
 *
 * Mirrors the file-system discipline of `LSMTree::compact`
 * (lsm_tree.rs:950-1156) and its crash-recovery replay
 * (lsm_tree.rs:424-438, run_compaction_action lsm_tree.rs:576-590), plus
 * the compaction trigger policy (tasks/compaction.rs:35-102), so that the
 * reference's artifact semantics (filenames `{index:020}.{ext}`
 * lsm_tree.rs:284-288, `.compact_*` staging files, the `.compact_action`
 * bincode journal with deletes-then-renames replay) keep working
 * unmodified above the GPU engine.
 *
 * Bloom: the reference's `.bloom` bytes are unpinnable (bloomfilter
 * v1.0.12 embeds random SipHash keys — SURVEY.md §8c); this layer writes
 * a behaviorally equivalent filter (zero false negatives, ~1% fp) in the
 * engine's own format ("DBLM" header), checked via dbeel_bloom_contains.
 */
#ifndef DBEEL_LSM_H
#define DBEEL_LSM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Compact the runs at `indices` in `dir` into `output_index`, with the
 * reference's full artifact discipline:
 *   read {i:020}.data/.index -> GPU merge -> write
 *   {out:020}.compact_data/.compact_index (+ .compact_bloom when total
 *   input data > sstable_bloom_min_size, lsm_tree.rs:1026-1034) ->
 *   write {out:020}.compact_action journal (renames + deletes) ->
 *   perform renames -> delete inputs -> delete journal
 *   (lsm_tree.rs:1070-1153).
 * device: HIP ordinal. Returns 0 or a dbeel_gpu error code. */
int dbeel_lsm_compact(const char* dir, const uint64_t* indices,
                      size_t n_indices, uint64_t output_index,
                      int keep_tombstones, int device,
                      uint64_t sstable_bloom_min_size,
                      uint64_t* out_entries_written);

/* dbeel_lsm_compact for inputs of any size: same contract, same staging
 * files, journal, crash hook (DBEEL_LSM_CRASH_AFTER_JOURNAL), renames and
 * deletes — the directory ends byte-identical to dbeel_lsm_compact's, the
 * .bloom included — but the device half is dbeel_gpu_compact_into
 * (include/dbeel_gpu.h): the inputs are read into buffers this call
 * page-locks, the output is fetched into page-locked buffers sized at the
 * inputs' summed lengths (which bound it, so the fetch cannot be refused),
 * slices are pipelined, and the filter — gated by
 * total input data > sstable_bloom_min_size exactly as above — is built
 * across slices. max_resident_bytes bounds one slice's input (0 = from the
 * device's free memory); inputs that fit run as one slice. Everything is
 * unpinned before the call returns. device < 0 is DBEEL_ERR_INVALID_ARG
 * before any file is read. */
int dbeel_lsm_compact_stream(const char* dir, const uint64_t* indices,
                             size_t n_indices, uint64_t output_index,
                             int keep_tombstones, int device,
                             uint64_t max_resident_bytes,
                             uint64_t sstable_bloom_min_size,
                             uint64_t* out_entries_written);

/* Replay any {n:020}.compact_action journals in dir: per journal, deletes
 * first (if present), then renames (if source present), then remove the
 * journal — idempotent compaction completion after a crash
 * (lsm_tree.rs:424-438, 576-590). Returns number of journals replayed in
 * *out_replayed (may be NULL). */
int dbeel_lsm_replay(const char* dir, uint32_t* out_replayed);

/* The compaction trigger policy of tasks/compaction.rs:35-102: discover
 * sstables ({i:020}.index), group by leading_zeros(entry_count), promote
 * groups whose combined count reaches a bigger size class, compact every
 * group with >= max(2, compaction_factor) members into the next odd
 * output index (+2 per group). Tombstones are dropped only when a group
 * covers EVERY live sstable: the reference's keep_tombstones = (i > 0)
 * over a HashMap enumeration (tasks/compaction.rs:82-92) is
 * nondeterministic and can resurrect deleted keys when a promoted group
 * of new runs enumerates first; this port implements the "only on the
 * final level" intent deterministically and safely. */
int dbeel_lsm_compact_tree(const char* dir, uint64_t compaction_factor,
                           int device, uint64_t sstable_bloom_min_size,
                           uint32_t* out_n_compactions);

/* Major compaction: merge EVERY live sstable in dir into one run at the
 * next odd output index, dropping tombstones (safe: nothing outside the
 * group can resurrect a deleted key). Bounds the tombstone buildup that
 * the conservative full-coverage rule in dbeel_lsm_compact_tree can
 * otherwise let accumulate (a steady-state tree may never form a
 * full-coverage group on its own — ADVICE r01); call periodically or
 * when space amplification matters. No-op (0 compactions) when fewer
 * than 2 sstables exist. */
int dbeel_lsm_major_compact(const char* dir, int device,
                            uint64_t sstable_bloom_min_size,
                            uint64_t* out_entries_written);

/* Membership test against an engine-format bloom file's bytes.
 * *out = 1 if possibly present, 0 if definitely absent. */
int dbeel_bloom_contains(const uint8_t* bloom_bytes, size_t bloom_len,
                         const uint8_t* key, size_t key_len, int* out);

/* Open a resident reader (include/dbeel_gpu.h) over every live sstable in
 * dir: discovers {i:020}.index in ascending order, reads .data/.index and
 * the .bloom when it exists. out_indices (capacity 64) maps hit.run back
 * to the sstable index; *out_n is the number of runs. Never mutates the
 * directory: a pending {n:020}.compact_action journal returns
 * DBEEL_ERR_IO (replay first), more than 64 sstables
 * DBEEL_ERR_INVALID_ARG (compact first). Close with
 * dbeel_gpu_reader_close. */
struct dbeel_gpu_reader;
int dbeel_lsm_reader_open(const char* dir, int device,
                          struct dbeel_gpu_reader** out,
                          uint64_t* out_indices, size_t* out_n);

/* Keep an open reader in step with its directory instead of reopening it.
 * indices[] is the caller's array from dbeel_lsm_reader_open (capacity
 * 64), *n its length; both are updated on success and left alone on
 * failure. After either call the reader answers exactly as a fresh
 * dbeel_lsm_reader_open of the directory would.
 *
 * reader_add: a flush wrote sstable_index (lsm_tree.rs:901-915). Reads
 * {i:020}.data/.index (+ .bloom if present) and inserts the run at its
 * ascending-index position; an index already present is
 * DBEEL_ERR_INVALID_ARG. (The reference appends a flushed table to the end
 * of its list and sorts only at the next compaction or restart,
 * lsm_tree.rs:903-912,1136 — documented divergence)
 *
 * reader_compact: dbeel_lsm_compact with the read-and-upload half replaced
 * by a compaction of the runs the reader already holds
 * (lsm_tree.rs:1113-1145): compact on the device -> staging files ->
 * journal -> renames -> swap the reader's list -> delete inputs -> remove
 * the journal. The directory ends byte-for-byte as dbeel_lsm_compact
 * leaves it; the bloom gate compares the compacted runs' data bytes with
 * sstable_bloom_min_size. A compact_indices entry not in indices, or an
 * output_index that is live and not itself compacted, is
 * DBEEL_ERR_INVALID_ARG. Any failure before the swap leaves the reader
 * answering from the old list. With DBEEL_LSM_CRASH_AFTER_JOURNAL set it
 * stops after the journal as dbeel_lsm_compact does (reader and indices
 * unchanged): the directory then needs dbeel_lsm_replay and the reader a
 * reopen.
 *
 * reader_flush: the flush itself (lsm_tree.rs:850-915) instead of
 * reader_add after a host-side flush. The write batch (the arrays of
 * dbeel_gpu_reader_write_batch, arrival order) is sorted, deduplicated and
 * encoded on the device into a new table at sstable_index's
 * ascending-index position, and the run is written as
 * {sstable_index:020}.data / .index under their final names — no .bloom:
 * the reference's flush passes None. An index already present is
 * DBEEL_ERR_INVALID_ARG before anything is written; a file that cannot be
 * written is DBEEL_ERR_IO, with the table taken out of the reader again and
 * what was written removed. n_writes == 0 writes nothing and changes
 * nothing.
 *
 * reader_memtable_flush: the flush of the reader's resident memtable
 * (dbeel_gpu_reader_put, include/dbeel_gpu.h). dbeel_gpu_reader_memtable_fetch
 * -> {sstable_index:020}.data / .index under their final names, no .bloom
 * -> dbeel_gpu_reader_memtable_flush(out = NULL) -> sstable_index appended
 * to indices. sstable_index must exceed every index held — the flushed
 * table has to be the newest both in the reader and after a reopen —
 * otherwise DBEEL_ERR_INVALID_ARG before anything is written. A file that
 * cannot be written is DBEEL_ERR_IO: what was written is removed, and the
 * reader and the memtable stay untouched (which is why the bytes are
 * fetched first). An empty memtable writes nothing. The write-ahead log
 * stays with the caller. */
int dbeel_lsm_reader_memtable_flush(const char* dir,
                                    struct dbeel_gpu_reader* reader,
                                    uint64_t* indices, size_t* n,
                                    uint64_t sstable_index);
int dbeel_lsm_reader_add(const char* dir, struct dbeel_gpu_reader* reader,
                         uint64_t* indices, size_t* n,
                         uint64_t sstable_index);
int dbeel_lsm_reader_flush(const char* dir, struct dbeel_gpu_reader* reader,
                           uint64_t* indices, size_t* n,
                           uint64_t sstable_index, uint64_t n_writes,
                           const uint8_t* keys, const uint64_t* key_offsets,
                           const uint8_t* values,
                           const uint64_t* value_offsets,
                           const uint8_t* timestamps);
int dbeel_lsm_reader_compact(const char* dir, struct dbeel_gpu_reader* reader,
                             uint64_t* indices, size_t* n,
                             const uint64_t* compact_indices, size_t n_compact,
                             uint64_t output_index, int keep_tombstones,
                             uint64_t sstable_bloom_min_size,
                             uint64_t* out_entries_written);

#ifdef __cplusplus
}
#endif
#endif /* DBEEL_LSM_H */
