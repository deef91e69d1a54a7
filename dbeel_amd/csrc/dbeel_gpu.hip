/* dbeel_gpu.hip — MI355X-native (gfx950/CDNA4) SSTable compaction engine.
 *
 * Implements include/dbeel_gpu.h: the drop-in replacement for dbeel's
 * LSMTree::compact hot loop (reference lsm_tree.rs:950-1156; semantics
 * restated in the header). This is a from-scratch GPU design, not a port of
 * the reference's heap loop:
 *
 *   k_prepare    : validates every entry (bounds + bincode field
 *                  cross-check + EntryWriter density; corrupt input
 *                  errors loudly where the reference silently truncates)
 *                  and extracts the dense key-prefix (8 B) and tiered
 *                  suffix-aux arrays (16/48/64 B: key bytes 8.., klen,
 *                  staged i128 ts in the duplicate-prone tiers) the
 *                  merge runs on. Rangeable for streamed ingest.
 *   k_corank     : block-cooperative merge-path co-ranking — for every
 *                  run pair WITHIN a job, diagonal-partitioned
 *                  2048-position windows; blocks stage both prefix
 *                  segments into LDS coalesced and walk CORANK_STEPS
 *                  merged positions per thread (a window's prefix-tied
 *                  pairs are listed in LDS and settled by the whole
 *                  block ahead of the walk), recording crossranks
 *                  (order = key bytes asc, timestamp i128 asc, run index
 *                  asc — lsm_tree.rs:52-71 + mod.rs:75-81) and
 *                  newest-wins supersession flags (lsm_tree.rs:1041-1044).
 *   k_rankreduce : crossranks -> job-local rank (+ job entry base);
 *                  winner/tombstone rules; strict-sortedness check
 *                  (flush invariant, lsm_tree.rs:925-946); one 16-B
 *                  rank-indexed record (keep flag in src bit 63); in the
 *                  job path's packed mode also the packed (count, bytes)
 *                  sum of every 2048-rank tile.
 *   k_tilebase   : the tile sums -> exclusive tile bases (one block).
 *   k_emit_tile  : one block per rank tile scans its tile from the base:
 *                  output .index records (offset/key_size/full_size,
 *                  entry_writer.rs:79-87) + compacted source map + the
 *                  step totals record that winmap/copy read on-device +
 *                  the copy's window map where no survivor is larger
 *                  than a window.
 *   scans/k_emit : everywhere else (jobs past the packing bounds, reader,
 *                  memtable, batch and scan paths): two rocPRIM
 *                  exclusive scans (transform iterators, plain u64/u32 +
 *                  plus to stay on the decoupled-lookback fast path) ->
 *                  survivor byte offsets + positions, then k_emit;
 *                  DBEEL_SCAN_MODE=rocprim: one packed scan +
 *                  k_emit_packed on the job path, for A/B.
 *   k_winmap/k_copy : (k_winmap only when emit did not fill the map)
 *                  verbatim survivor copy, balanced by DESTINATION
 *                  granule (16-B granules per lane, window/grid geometry
 *                  picked per survivor size from interleaved A/Bs, LDS
 *                  granule->entry map) so throughput is independent of
 *                  entry size; full windows gather granule values into
 *                  registers before storing; aligned non-temporal 16-B
 *                  stores, unaligned 16-B loads, boundary granules via
 *                  16-B two-load blends.
 *   k_scanflag   : the AsyncIter migration scan filter (murmur3 hash
 *                  ranges + key bounds — lsm_tree.rs:141-282,
 *                  tasks/migration.rs:54-60).
 *   k_encode_*   : the memtable-flush run encoder (lsm_tree.rs:925-946).
 *   k_reader_*   : the resident table reader (LSMTree::get over the
 *                  sstables, lsm_tree.rs:674-723): open-time validation
 *                  + prefix array, batched search with the on-device
 *                  bloom prefilter, value gather; k_reader_adopt turns
 *                  a compaction output into a resident table (prefixes
 *                  + filter bits in one pass) for the live table list;
 *                  k_reader_scan_bounds/_flag/_emit page the migration
 *                  scan over the resident tables into caller buffers;
 *                  k_reader_scan_shadow (snapshot scans with
 *                  DBEEL_SCAN_NEWEST_ONLY) drops the candidates whose key
 *                  a later table or the memtable holds.
 *   k_batch_*    : the memtable + flush for the reader: an unsorted
 *                  write batch is ordered (one rocPRIM merge sort on
 *                  (prefix, key, arrival); or a radix sort on the prefix
 *                  plus a merge sort of the prefix-tied writes only),
 *                  deduplicated (last arrival wins) and encoded through
 *                  the arrival index straight into a new resident table.
 *   k_page_*     : a scan page as that batch (put_entries, scan_apply):
 *                  every entry validated, the masked-out ones compacted
 *                  away, the same order stage with keys read in place,
 *                  survivors copied verbatim or rewritten as tombstones.
 *   k_index_rebase / k_bloom_hash / k_bloom_fill : compaction into
 *                  caller buffers in pipelined key slices — index offsets
 *                  rebased on the device on the way in (-slice start) and
 *                  out (+running output offset, in scratch), the "DBLM"
 *                  filter built across slices from appended hashes.
 *   host side   : resident jobs, batched independent jobs (one launch
 *                  set, per-job output slicing), streamed pinned ingest
 *                  with copy/compute overlap, sliced compaction for
 *                  inputs larger than HBM, device bloom build.
 *
 * All integer/byte work, HBM-bandwidth bound; MFMA unused by design
 * (BASELINE.json north_star).
 *
 * Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC dbeel_gpu.hip
 *        -o libdbeel_gpu.so
 */
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <new>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/dbeel_gpu.h"
#include "engine_internal.h"

#define MAX_RUNS 64
#define JOB_ERR_WORDS 4 /* u32 words of a job's d_err ahead of the tile sums */

static thread_local char g_err[512];

static void set_err(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

extern "C" const char* dbeel_gpu_last_error(void) { return g_err; }

/* Library-internal: lets the file-level layer (dbeel_lsm.cpp, linked into
 * the same .so) report through dbeel_gpu_last_error. Not exported. */
extern "C" void dbeel_set_last_error(const char* msg) {
    set_err("%s", msg);
}

/* The one check macro: a failed HIP call sets the error text and returns
 * DBEEL_ERR_OOM / DBEEL_ERR_HIP from the enclosing function. What has to
 * be undone on the way out is the function's business, declared once as a
 * ScopeGuard. */
#define HIP_CHECK(call)                                                     \
    do {                                                                    \
        hipError_t _e = (call);                                             \
        if (_e != hipSuccess) {                                             \
            set_err("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e),  \
                    __FILE__, __LINE__);                                    \
            return (_e == hipErrorOutOfMemory) ? DBEEL_ERR_OOM              \
                                               : DBEEL_ERR_HIP;             \
        }                                                                   \
    } while (0)

/* Runs f when the scope ends, on every path out of it, unless dismissed. */
template <typename F>
struct ScopeGuard {
    F f;
    bool armed = true;
    explicit ScopeGuard(F fn) : f(fn) {}
    ScopeGuard(const ScopeGuard&) = delete;
    ScopeGuard& operator=(const ScopeGuard&) = delete;
    ~ScopeGuard() {
        if (armed) f();
    }
    void dismiss() { armed = false; }
};

/* The device argument of every entry point: there is no CPU fallback. */
static int check_device_arg(int device) {
    if (device >= 0) return DBEEL_OK;
    set_err("device must be >= 0 (no CPU fallback in the product library; "
            "the CPU restatement lives in oracle/liboracle.so and is test "
            "infrastructure only)");
    return DBEEL_ERR_INVALID_ARG;
}

/* Makes `device` the calling thread's HIP device: DBEEL_ERR_INVALID_ARG
 * for a negative one, DBEEL_ERR_NO_GPU when HIP cannot provide it. */
static int select_device(int device) {
    int rc = check_device_arg(device);
    if (rc) return rc;
    int ndev = 0;
    hipError_t de = hipGetDeviceCount(&ndev);
    if (de != hipSuccess || device >= ndev) {
        set_err("no usable HIP device %d (count=%d, %s)", device, ndev,
                hipGetErrorString(de));
        return DBEEL_ERR_NO_GPU;
    }
    HIP_CHECK(hipSetDevice(device));
    return DBEEL_OK;
}

/* The launch grid of every grid-stride kernel. */
static uint32_t pick_grid(uint64_t work_items, uint32_t block) {
    uint64_t blocks = (work_items + block - 1) / block;
    /* 256 CUs x 8 workgroups/CU = 2048; cap and grid-stride the rest */
    if (blocks > 2048) blocks = 2048;
    if (blocks == 0) blocks = 1;
    return (uint32_t)blocks;
}

/* ------------------------------------------------------------------ */
/* Device-side format view                                            */
/* ------------------------------------------------------------------ */

struct RunsDesc {
    const uint8_t* data[MAX_RUNS];
    const uint8_t* index[MAX_RUNS];
    uint64_t data_len[MAX_RUNS];
    uint64_t count[MAX_RUNS];       /* entries per run                  */
    uint64_t entry_base[MAX_RUNS];  /* exclusive prefix sum of count    */
    uint8_t job_lo[MAX_RUNS];       /* run-range [lo, hi) of the        */
    uint8_t job_hi[MAX_RUNS];       /* INDEPENDENT job owning run r     */
    int n_runs;
    uint64_t total;                 /* sum of count                     */
};

struct EView {
    const uint8_t* raw;
    const uint8_t* key;
    uint64_t klen;
    uint64_t off;
    uint32_t key_size, full_size;
};

__device__ __forceinline__ uint64_t ld_u64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
__device__ __forceinline__ uint32_t ld_u32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

/* Loads index record + key view. Returns false on a corrupt record, and
 * then e.raw / e.key are not set: nothing may be read through them. This
 * is the only bounds check there is — off and full_size come from the
 * input, so it is written so that no sum of them can wrap. */
__device__ __forceinline__ bool load_entry(const RunsDesc& R, int r,
                                           uint64_t i, EView& e) {
    const uint8_t* rec = R.index[r] + i * 16;
    e.off = ld_u64(rec);
    e.key_size = ld_u32(rec + 8);
    e.full_size = ld_u32(rec + 12);
    const uint64_t dlen = R.data_len[r];
    if (e.key_size < 8 || e.full_size < 32 ||
        (uint64_t)e.key_size + 24 > e.full_size ||
        e.off > dlen || e.full_size > dlen - e.off)
        return false;
    e.raw = R.data[r] + e.off;
    e.klen = e.key_size - 8;
    e.key = e.raw + 8;
    return true;
}

/* Lexicographic compare of key byte strings (Vec<u8> cmp, mod.rs:75-81). */
__device__ __forceinline__ int cmp_keys(const uint8_t* a, uint64_t la,
                                        const uint8_t* b, uint64_t lb) {
    uint64_t n = la < lb ? la : lb;
    uint64_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t va = ld_u64(a + i), vb = ld_u64(b + i);
        if (va != vb) {
            va = __builtin_bswap64(va);
            vb = __builtin_bswap64(vb);
            return va < vb ? -1 : 1;
        }
    }
    if (i < n) {
        uint64_t rem = n - i;
        uint64_t va = 0, vb = 0;
        for (uint64_t j = 0; j < rem; j++) {  /* <= 7 bytes */
            va |= (uint64_t)a[i + j] << (8 * j);
            vb |= (uint64_t)b[i + j] << (8 * j);
        }
        if (va != vb) {
            va = __builtin_bswap64(va);
            vb = __builtin_bswap64(vb);
            return va < vb ? -1 : 1;
        }
    }
    return la < lb ? -1 : (la > lb ? 1 : 0);
}

/* Timestamp: trailing i128 LE (utils/timestamp_nanos.rs:6-11). */
__device__ __forceinline__ void load_ts(const EView& e, uint64_t& lo,
                                        int64_t& hi) {
    lo = ld_u64(e.raw + e.full_size - 16);
    int64_t h;
    __builtin_memcpy(&h, e.raw + e.full_size - 8, 8);
    hi = h;
}

/* ------------------------------------------------------------------ */
/* Kernels                                                            */
/* ------------------------------------------------------------------ */

/* err codes stored in the device flag */
#define DERR_CORRUPT 1u
#define DERR_UNSORTED 2u

/* Big-endian key prefix: the first min(8, klen) key bytes, zero-padded,
 * byteswapped so u64 comparison == lexicographic byte comparison of those
 * bytes. pfx(a) != pfx(b) implies sign(u64 cmp) == sign(key cmp); equality
 * requires the full comparator (length / tail bytes / timestamp). */
__device__ __forceinline__ uint64_t key_prefix(const uint8_t* key,
                                               uint64_t klen) {
    uint64_t v = 0;
    if (klen >= 8) {
        v = ld_u64(key);
    } else {
        for (uint64_t j = 0; j < klen; j++) v |= (uint64_t)key[j] << (8 * j);
    }
    return __builtin_bswap64(v);
}

/* The run that owns global entry g (<= 64 runs: linear scan on the cached
 * desc). */
__device__ __forceinline__ int run_of(const RunsDesc& R, uint64_t g) {
    int r = 0;
    while (r + 1 < R.n_runs && g >= R.entry_base[r + 1]) r++;
    return r;
}

/* What k_prepare and k_reader_prepare ask of an entry that load_entry
 * accepted: the bincode length fields agree with the index record
 * (read_next_entry, lsm_tree.rs:1158-70), and the successor's offset is
 * monotone and does not overlap (EntryWriter appends —
 * entry_writer.rs:71-98; the streamed-ingest chunking relies on it). */
__device__ __forceinline__ bool entry_consistent(const RunsDesc& R, int r,
                                                 uint64_t i,
                                                 const EView& e) {
    if (ld_u64(e.raw) != e.klen ||
        ld_u64(e.raw + 8 + e.klen) != (uint64_t)e.full_size - 32 - e.klen)
        return false;
    return i + 1 >= R.count[r] ||
           e.off + e.full_size <= ld_u64(R.index[r] + (i + 1) * 16);
}

/* ---- Search inside one run: bisect the dense prefix array, then settle
 * the equal-prefix stretch (zero padding, bytes past 8, length) with full
 * key compares on the blob — never a walk. ---- */

/* First i in [0, n) with P[i] >= qp; n when there is none. */
__device__ __forceinline__ uint64_t pfx_lower_bound(const uint64_t* P,
                                                    uint64_t n,
                                                    uint64_t qp) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        uint64_t mid = (lo + hi) >> 1;
        if (P[mid] < qp)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

/* First i in [lo, n) with P[i] > qp; n when there is none. */
__device__ __forceinline__ uint64_t pfx_upper_bound(const uint64_t* P,
                                                    uint64_t lo, uint64_t n,
                                                    uint64_t qp) {
    uint64_t hi = n;
    while (lo < hi) {
        uint64_t mid = (lo + hi) >> 1;
        if (P[mid] <= qp)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

/* First entry in [lo, hi) of run r whose key is >= (key, klen); hi when
 * there is none. A record that fails to load narrows from above: on
 * corrupt input the search degrades safely. */
__device__ __forceinline__ uint64_t blob_lower_bound(const RunsDesc& R, int r,
                                                     uint64_t lo, uint64_t hi,
                                                     const uint8_t* key,
                                                     uint64_t klen) {
    while (lo < hi) {
        uint64_t mid = (lo + hi) >> 1;
        EView m;
        if (!load_entry(R, r, mid, m)) {
            hi = mid;
            continue;
        }
        if (cmp_keys(m.key, m.klen, key, klen) < 0)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

/* Dense per-entry search record: the key's SUFFIX bytes (8..8+KB,
 * zero-padded — the first 8 live in the pfx array, never duplicated here)
 * plus the key length. Prefix-tied comparisons read THIS instead of the
 * scattered multi-GiB data blob. Timestamps are NOT staged: the (ts, run)
 * tie-break only fires on fully EQUAL keys (true cross-run duplicates),
 * which read the two entries' trailing i128 from the blob — trading a
 * rare scattered read for a dense 16-byte write saved on EVERY entry
 * (cfg3: 1.0 GB of prep traffic). The tier (KB = 12/28/60 -> 16/32/64-B
 * records) is picked per job from the max key_size in the uploaded
 * indexes; longer keys stay CORRECT in any tier (blob fallback when two
 * keys tie through 8+KB bytes), smaller tiers are purely a traffic
 * optimization. */
template <int KB, bool TS> struct AuxT;
template <int KB> struct AuxT<KB, false> {
    uint8_t key[KB]; /* key bytes 8..8+KB, zero-padded */
    uint32_t klen;
};
template <int KB> struct AuxT<KB, true> {
    uint8_t key[KB];
    uint32_t klen;
    uint32_t rsv;
    uint64_t ts_lo; /* timestamp i128 LE halves — staged for tiers where
                       cross-run duplicates are expected so the (ts, run)
                       tie-break stays dense instead of 2 scattered blob
                       lines per comparison (PMC r02: blob ts reads cost
                       corank +1.3 GB on cfg3) */
    int64_t ts_hi;
};
static_assert(sizeof(AuxT<12, false>) == 16, "tier-0 aux must be 16B");
static_assert(sizeof(AuxT<24, true>) == 48, "tier-1 aux must be 48B");
static_assert(sizeof(AuxT<40, true>) == 64, "tier-2 aux must be 64B");

/* Host-side tier dispatch: calls f with the <KB, TS> of a job's aux_kind
 * (0: 16-B, 1: 48-B, 2: 64-B records) as compile-time constants, for the
 * templated launches:
 *   with_aux_tier(kind, [&](auto tier) {
 *       using T = decltype(tier);  ... k_x<T::KB, T::TS> ... }); */
template <int KB_, bool TS_> struct AuxTier {
    static constexpr int KB = KB_;
    static constexpr bool TS = TS_;
    using Rec = AuxT<KB_, TS_>;
};
template <typename F> static void with_aux_tier(int kind, F&& f) {
    switch (kind) {
        case 0: f(AuxTier<12, false>{}); break;
        case 1: f(AuxTier<24, true>{}); break;
        case 2: f(AuxTier<40, true>{}); break;
    }
}

/* Key-only compare of entries A=(rA,iA), B=(rB,iB) via suffix records.
 * PRECONDITION: pfx(A) == pfx(B) (every caller compares pfx first), so
 * the first min(8, klen) key bytes already agree and zero-padding in pfx
 * is consistent: equality there with different klen means one key is a
 * zero-extension of the other within 8 bytes, which the klen comparison
 * below orders correctly (a strict prefix sorts first). */
/* The record part of that compare: works on two aux records wherever they
 * live (global memory, or registers a caller loaded ahead of need). Sets
 * `deep` and returns 0 when both keys run past the staged 8+KB bytes and
 * tie through them — only the blob can order those. */
template <int KB, bool TS>
__device__ __forceinline__ int cmp_keys_rec(const AuxT<KB, TS>& a,
                                            const AuxT<KB, TS>& b,
                                            bool& deep) {
    deep = false;
    uint32_t la = a.klen, lb = b.klen;
    uint32_t n = la < lb ? la : lb;
    uint32_t ns = n > 8 ? n - 8 : 0; /* suffix bytes to compare */
    if (ns > KB) ns = KB;
    #pragma unroll
    for (uint32_t i = 0; i < KB; i += 8) {
        if (i >= ns) break;
        uint64_t va, vb;
        __builtin_memcpy(&va, a.key + i, 8);
        __builtin_memcpy(&vb, b.key + i, 8);
        if (i + 8 > ns) { /* mask the tail; reading into klen is masked
                             off (and pad bytes are zero anyway) */
            uint64_t mask = (~0ull) >> (8 * (i + 8 - ns));
            va &= mask;
            vb &= mask;
        }
        if (va != vb) {
            va = __builtin_bswap64(va);
            vb = __builtin_bswap64(vb);
            return va < vb ? -1 : 1;
        }
    }
    if (la > (uint32_t)(8 + KB) && lb > (uint32_t)(8 + KB)) {
        deep = true;
        return 0;
    }
    return la < lb ? -1 : (la > lb ? 1 : 0);
}

template <int KB, bool TS>
__device__ __forceinline__ int cmp_keys_sfx(const RunsDesc& R,
                                            const AuxT<KB, TS>* aux, int rA,
                                            uint64_t iA, int rB,
                                            uint64_t iB) {
    const AuxT<KB, TS>* a = aux + R.entry_base[rA] + iA;
    const AuxT<KB, TS>* b = aux + R.entry_base[rB] + iB;
    bool deep;
    int c = cmp_keys_rec<KB, TS>(*a, *b, deep);
    if (deep) {
        /* rare: long keys tied through the staged 8+KB bytes */
        EView ea, eb;
        if (!load_entry(R, rA, iA, ea) || !load_entry(R, rB, iB, eb))
            return -1; /* corrupt input flagged elsewhere; value discarded */
        return cmp_keys(ea.key, ea.klen, eb.key, eb.klen);
    }
    return c;
}

/* (timestamp, run index) tie-break from the blob — only reached on fully
 * equal keys (lsm_tree.rs:58-65 + mod.rs:75-81: ts i128 asc, then run
 * index asc). */
__device__ __forceinline__ int cmp_ts_run_blob(const RunsDesc& R, int rA,
                                               uint64_t iA, int rB,
                                               uint64_t iB) {
    EView a, b;
    if (!load_entry(R, rA, iA, a) || !load_entry(R, rB, iB, b))
        return rA < rB ? -1 : 1; /* corrupt flagged elsewhere; stable */
    uint64_t alo, blo;
    int64_t ahi, bhi;
    load_ts(a, alo, ahi);
    load_ts(b, blo, bhi);
    if (ahi != bhi) return ahi < bhi ? -1 : 1;
    if (alo != blo) return alo < blo ? -1 : 1;
    return rA < rB ? -1 : (rA > rB ? 1 : 0);
}

/* Full-order compare (key, timestamp, run index — lsm_tree.rs:52-71). */
template <int KB, bool TS>
__device__ __forceinline__ int cmp_sfx_full(const RunsDesc& R,
                                            const AuxT<KB, TS>* aux, int rA,
                                            uint64_t iA, int rB,
                                            uint64_t iB) {
    int c = cmp_keys_sfx<KB, TS>(R, aux, rA, iA, rB, iB);
    if (c) return c;
    if constexpr (TS) {
        const AuxT<KB, TS>* a = aux + R.entry_base[rA] + iA;
        const AuxT<KB, TS>* b = aux + R.entry_base[rB] + iB;
        if (a->ts_hi != b->ts_hi) return a->ts_hi < b->ts_hi ? -1 : 1;
        if (a->ts_lo != b->ts_lo) return a->ts_lo < b->ts_lo ? -1 : 1;
        return rA < rB ? -1 : (rA > rB ? 1 : 0);
    } else {
        return cmp_ts_run_blob(R, rA, iA, rB, iB);
    }
}

/* cmp_sfx_full that also reports whether the KEYS are equal, so a caller
 * that needs both answers about one pair (who goes first; is the other a
 * duplicate key) reads the pair's records once. Returns A < B. */
template <int KB, bool TS>
__device__ __forceinline__ bool tie_eval(const RunsDesc& R,
                                         const AuxT<KB, TS>* aux, int rA,
                                         uint64_t iA, int rB, uint64_t iB,
                                         bool& keq) {
    int c = cmp_keys_sfx<KB, TS>(R, aux, rA, iA, rB, iB);
    keq = (c == 0);
    if (c) return c < 0;
    if constexpr (TS) {
        const AuxT<KB, TS>* a = aux + R.entry_base[rA] + iA;
        const AuxT<KB, TS>* b = aux + R.entry_base[rB] + iB;
        if (a->ts_hi != b->ts_hi) return a->ts_hi < b->ts_hi;
        if (a->ts_lo != b->ts_lo) return a->ts_lo < b->ts_lo;
        return rA < rB;
    } else {
        return cmp_ts_run_blob(R, rA, iA, rB, iB) < 0;
    }
}

/* Merge-path split on diagonal d: the smallest s in [lo, hi] for which
 * A[s] < B[d-s-1] (full order) is false. pa(s) / pb(s) give the 8-byte
 * prefixes, full_lt(s, t) the full compare of A[s] with B[t].
 *
 * The prefixes decide wherever they can. Q(s) = pa(s) < pb(d-s-1) implies
 * the full predicate and is monotone like it, so a search on Q alone (ties
 * counted false) lands at or before the true split, and the steps between
 * the two are exactly the leading part of the stretch [s_Q, e) on which the
 * two prefixes are equal (pa rises and pb(d-s-1) falls with s, so that
 * stretch is contiguous and everything past it is "greater"). Full
 * compares, the only ones that leave the prefix array, settle that stretch:
 * one for a lone tied pair, a binary search otherwise. The result is the
 * split a search on the full predicate finds. */
template <typename T, typename PA, typename PB, typename FULL>
__device__ __forceinline__ T diag_split(T lo, T hi, T d, PA pa, PB pb,
                                        FULL full_lt) {
    const T hi0 = hi;
    while (lo < hi) {
        T mid = (lo + hi) >> 1;
        if (pa(mid) < pb(d - mid - 1))
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo < hi0 && pa(lo) == pb(d - lo - 1)) {
        T e = lo + 1;
        if (e < hi0 && pa(e) == pb(d - e - 1)) {
            T l = e + 1, h = hi0; /* first s past the equal stretch */
            while (l < h) {
                T m = (l + h) >> 1;
                if (pa(m) == pb(d - m - 1))
                    l = m + 1;
                else
                    h = m;
            }
            e = l;
        }
        T l = lo, h = e;
        while (l < h) {
            T m = (l + h) >> 1;
            if (full_lt(m, d - m - 1))
                l = m + 1;
            else
                h = m;
        }
        lo = l;
    }
    return lo;
}

/* Validates every entry (bounds + bincode field cross-check,
 * read_next_entry lsm_tree.rs:1158-70) and extracts the dense key-prefix
 * and aux arrays the merge runs on. Run sortedness is checked in
 * k_rankreduce (on the dense pfx/aux arrays). */
template <int KB, bool TS>
__global__ void k_prepare(RunsDesc R, uint64_t g0, uint64_t g1,
                          uint64_t* pfx, AuxT<KB, TS>* aux, uint32_t* err) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = g0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         g < g1; g += stride) {
        int r = run_of(R, g);
        uint64_t i = g - R.entry_base[r];
        EView e;
        if (!load_entry(R, r, i, e)) {
            atomicOr(err, DERR_CORRUPT);
            pfx[g] = 0;
            AuxT<KB, TS> z = {};
            aux[g] = z;
            continue;
        }
        pfx[g] = key_prefix(e.key, e.klen);
        AuxT<KB, TS> a;
        a.klen = (uint32_t)e.klen;
        if constexpr (TS) {
            a.rsv = 0;
            load_ts(e, a.ts_lo, a.ts_hi);
        }
        /* stage key SUFFIX bytes 8..8+KB, zero-padded. 8-byte chunked
         * copy; reading up to 7 bytes past the key is safe (the 8-byte
         * data_len field follows it inside the entry) and the over-read
         * is masked off */
        uint32_t nk = e.klen > 8 ? (uint32_t)e.klen - 8 : 0;
        if (nk > KB) nk = KB;
        if (nk >= KB) {
            /* full staged suffix (uniform-key workloads: cfg3's 32-B
             * keys fill the 24-B tier exactly) — no masking, straight
             * word copies (prepare measured 40% issue-stall-bound) */
            #pragma unroll
            for (uint32_t j = 0; j < KB; j += 8) {
                uint64_t v = ld_u64(e.key + 8 + j);
                uint32_t nb = (KB - j) < 8 ? (KB - j) : 8;
                __builtin_memcpy(a.key + j, &v, nb);
            }
        } else {
            #pragma unroll
            for (uint32_t j = 0; j < KB; j += 8) {
                uint64_t v = 0;
                if (j < nk) {
                    v = ld_u64(e.key + 8 + j);
                    if (j + 8 > nk)
                        v &= (~0ull) >> (8 * (j + 8 - nk));
                }
                uint32_t nb = (KB - j) < 8 ? (KB - j) : 8;
                __builtin_memcpy(a.key + j, &v, nb);
            }
        }
        aux[g] = a;
        if (!entry_consistent(R, r, i, e)) atomicOr(err, DERR_CORRUPT);
    }
}

/* ------------------------------------------------------------------ */
/* Crossranks by block-cooperative merge-path co-ranking               */
/*                                                                     */
/* For every run pair (a, b), the merged sequence (full order: key,    */
/* timestamp, run index — a strict total order, so no merge ties) is   */
/* partitioned into CORANK_BLOCK_POS-wide windows by diagonal binary   */
/* search. Each 256-thread block stages the two pfx segments of its    */
/* window into LDS with coalesced loads, sub-partitions the window     */
/* CORANK_STEPS merged positions per thread (diagonal search in LDS),  */
/* walks linearly, recording for every consumed entry its crossrank    */
/* into the opposite run (= the opposite cursor) and whether the       */
/* opposite run's next entry carries the same key (then it is later    */
/* in the order and supersedes it — the newest-wins dedup of           */
/* lsm_tree.rs:1041-1046). Work is (k-1)*N sequential LDS compares;    */
/* global traffic is one coalesced pass over pfx plus rare aux reads   */
/* on prefix ties (duplicate keys).                                    */
/*                                                                     */
/* cr layout: column-major, cr[s * total + g] = crossrank of entry g   */
/* into the s-th OTHER run of g's run (s = r2 < r ? r2 : r2-1), with   */
/* bit 31 = superseded flag. Every slot is written exactly once.       */
/* ------------------------------------------------------------------ */

#define CORANK_BLOCK 256
#define CORANK_STEPS 8
#define CORANK_BLOCK_POS (CORANK_BLOCK * CORANK_STEPS) /* 2048 */
/* A window's tie list (k_corank): one u32 per prefix-tied pair, the staged
 * slot x of run a in bits 0..10, the slot y of run b in bits 11..21, and,
 * once the pair is settled, bit 22 valid, 23 keys equal, 24 a first. */
#define TIE_XY_BITS 11
#define TIE_XY_MASK ((1u << (2 * TIE_XY_BITS)) - 1)
#define TIE_VALID (1u << 22)
#define TIE_KEQ (1u << 23)
#define TIE_AFIRST (1u << 24)
static_assert(CORANK_BLOCK_POS <= (1 << TIE_XY_BITS),
              "a staged slot must fit a tie-list field");
#define CR_LOSER 0x80000000u
#define CR_MASK 0x7FFFFFFFu

struct PairDesc {
    uint32_t a, b;
    uint64_t chunk_base; /* exclusive prefix sum of per-pair windows */
};

/* Window-corner diagonal searches, one THREAD per chunk — fully
 * parallel. Previously each corank block ran its start/end corner
 * searches on 2 threads while the other 254 waited at the barrier
 * (corank measured 83% wave-parked); precomputing corners removes the
 * serial section. d_corners[t] = the merged-path `ia` at chunk t's
 * starting diagonal; a chunk's END corner is the next chunk's start
 * (same pair) or the pair's (Na, Nb) terminus. */
template <int KB, bool TS>
__global__ void k_corners(RunsDesc R, const uint64_t* pfx,
                          const AuxT<KB, TS>* aux, const PairDesc* pairs,
                          uint32_t n_pairs, uint64_t total_chunks,
                          uint64_t* corners) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         t < total_chunks; t += stride) {
        uint32_t plo = 0, phi = n_pairs;
        while (plo < phi) {
            uint32_t mid = (plo + phi) >> 1;
            if (pairs[mid].chunk_base <= t)
                plo = mid + 1;
            else
                phi = mid;
        }
        const PairDesc P = pairs[plo - 1];
        const int a = (int)P.a, b = (int)P.b;
        const uint64_t Na = R.count[a], Nb = R.count[b];
        const uint64_t* gpa = pfx + R.entry_base[a];
        const uint64_t* gpb = pfx + R.entry_base[b];
        uint64_t diag = (t - P.chunk_base) * CORANK_BLOCK_POS;
        uint64_t slo = diag > Nb ? diag - Nb : 0;
        uint64_t shi = diag < Na ? diag : Na;
        slo = diag_split<uint64_t>(
            slo, shi, diag, [&](uint64_t s) { return gpa[s]; },
            [&](uint64_t s) { return gpb[s]; },
            [&](uint64_t s, uint64_t u) {
                return cmp_sfx_full<KB, TS>(R, aux, a, s, b, u) < 0;
            });
        corners[t] = slo;
    }
}

template <int KB, bool TS, int BLK = CORANK_BLOCK>
__global__ __launch_bounds__(BLK) void k_corank(
    RunsDesc R, const uint64_t* pfx, const AuxT<KB, TS>* aux,
    const PairDesc* pairs, uint32_t n_pairs, uint64_t total_chunks,
    const uint64_t* corners, uint32_t* cr) {
    constexpr int STEPS = CORANK_BLOCK_POS / BLK; /* positions/thread */
    __shared__ uint64_t s_pfx[CORANK_BLOCK_POS + 2];
    __shared__ uint32_t s_cr[CORANK_BLOCK_POS]; /* staged crossranks:
        [0..lenA) for run a, [lenA..lenA+lenB) for run b — each block's
        output ranges are contiguous, so results are staged here and
        written back coalesced (direct interleaved 4-B stores measured
        3x write amplification from line RMW thrash) */
    for (uint64_t t = blockIdx.x; t < total_chunks; t += gridDim.x) {
        /* largest pair with chunk_base <= t (uniform across the block) */
        uint32_t plo = 0, phi = n_pairs;
        while (plo < phi) {
            uint32_t mid = (plo + phi) >> 1;
            if (pairs[mid].chunk_base <= t)
                plo = mid + 1;
            else
                phi = mid;
        }
        /* next pair's base bounds this pair's chunk range */
        uint64_t pair_end_chunk =
            (plo < n_pairs) ? pairs[plo].chunk_base : total_chunks;
        const PairDesc P = pairs[plo - 1];
        const int a = (int)P.a, b = (int)P.b;
        const uint64_t Na = R.count[a], Nb = R.count[b];
        const uint64_t* gpa = pfx + R.entry_base[a];
        const uint64_t* gpb = pfx + R.entry_base[b];
        uint64_t diag0 = (t - P.chunk_base) * CORANK_BLOCK_POS;
        uint64_t diag1 = diag0 + CORANK_BLOCK_POS;
        if (diag1 > Na + Nb) diag1 = Na + Nb;

        /* window corners precomputed by k_corners */
        const uint64_t iaS = corners[t];
        const uint64_t ibS = diag0 - iaS;
        const uint64_t iaE = (t + 1 < pair_end_chunk) ? corners[t + 1] : Na;
        const uint64_t ibE = diag1 - iaE;
        const uint32_t lenA = (uint32_t)(iaE - iaS);
        const uint32_t lenB = (uint32_t)(ibE - ibS);

        /* stage both pfx segments (coalesced); sA = s_pfx[0..lenA),
         * sB = s_pfx[lenA..lenA+lenB) */
        for (uint32_t u = threadIdx.x; u < lenA; u += BLK)
            s_pfx[u] = gpa[iaS + u];
        for (uint32_t u = threadIdx.x; u < lenB; u += BLK)
            s_pfx[lenA + u] = gpb[ibS + u];
        __syncthreads();
        const uint64_t* sA = s_pfx;
        const uint64_t* sB = s_pfx + lenA;

        /* per-thread sub-window: local diagonal search inside LDS */
        uint32_t L = lenA + lenB;
        uint32_t d = threadIdx.x * STEPS;
        uint32_t ja = 0, jb = 0, dend = 0;
        /* Scout: a prefix-only two-pointer sweep over the positions this
         * thread walks notes every pair with equal prefixes. The sweep
         * consumes both entries of such a pair, so a thread notes at most
         * STEPS/2 of them and a window at most CORANK_BLOCK_POS/2. */
        constexpr int MAXP = STEPS / 2;
        uint32_t tie[MAXP]; /* noted pairs, then their settled entries */
        uint32_t ntie = 0;
        #pragma unroll
        for (int m = 0; m < MAXP; m++)
            tie[m] = TIE_XY_MASK; /* no pair: x + y < CORANK_BLOCK_POS */
        if (d < L) {
            uint32_t slo = d > lenB ? d - lenB : 0;
            uint32_t shi = d < lenA ? d : lenA;
            slo = diag_split<uint32_t>(
                slo, shi, d, [&](uint32_t s) { return sA[s]; },
                [&](uint32_t s) { return sB[s]; },
                [&](uint32_t s, uint32_t u) {
                    return cmp_sfx_full<KB, TS>(R, aux, a, iaS + s, b,
                                                ibS + u) < 0;
                });
            ja = slo, jb = d - slo;
            dend = d + STEPS;
            if (dend > L) dend = L;
            uint32_t x = ja, y = jb, c = d;
            while (c < dend && x < lenA && y < lenB) {
                uint64_t pa = sA[x], pb = sB[y];
                if (pa < pb) {
                    x++, c++;
                } else if (pa > pb) {
                    y++, c++;
                } else {
                    #pragma unroll
                    for (int m = 0; m < MAXP; m++)
                        if ((int)ntie == m) tie[m] = x | (y << TIE_XY_BITS);
                    ntie++, x++, y++, c += 2;
                }
            }
        }

        /* The window's tie list, in ascending x: a block scan of the
         * per-thread counts places each thread's pairs. The list lives in
         * s_cr, which is free until the walk and holds twice the at most
         * CORANK_BLOCK_POS/2 entries; the per-wave totals (<= 64 * MAXP
         * each) take the two slack words of s_pfx, which nothing else
         * touches. Every thread of the block takes part, with or without
         * positions of its own. */
        constexpr int NWAVE = BLK / 64;
        static_assert(NWAVE * sizeof(uint16_t) <= 2 * sizeof(uint64_t) &&
                          64 * MAXP <= 0xFFFF,
                      "wave totals must fit the slack of s_pfx");
        uint32_t* s_list = s_cr;
        uint16_t* s_wtot = (uint16_t*)(s_pfx + CORANK_BLOCK_POS);
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        uint32_t incl = ntie;
        #pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            uint32_t up = __shfl_up(incl, o);
            if (lane >= (uint32_t)o) incl += up;
        }
        if (lane == 63) s_wtot[wave] = incl;
        __syncthreads();
        uint32_t lbase = incl - ntie, n_list = 0;
        #pragma unroll
        for (int w = 0; w < NWAVE; w++) {
            uint32_t wt = s_wtot[w];
            if ((uint32_t)w < wave) lbase += wt;
            n_list += wt;
        }
        /* n_list is the same in every thread: a window without prefix
         * ties takes none of the barriers below */
        if (n_list) {
            #pragma unroll
            for (int m = 0; m < MAXP; m++)
                if (m < (int)ntie) s_list[lbase + m] = tie[m];
            __syncthreads();
            /* Settle: the block's threads share the list evenly, whoever
             * noted the pair. Consecutive entries index nearly consecutive
             * aux records of both runs. Each pair is settled once, ahead
             * of the walk, so the walk's serial steps do not each wait on
             * a dependent global load. Keys tied through the staged bytes
             * (deep) stay unsettled. */
            const AuxT<KB, TS>* xa = aux + R.entry_base[a] + iaS;
            const AuxT<KB, TS>* xb = aux + R.entry_base[b] + ibS;
            for (uint32_t u = threadIdx.x; u < n_list; u += BLK) {
                uint32_t e = s_list[u];
                uint32_t hx = e & ((1u << TIE_XY_BITS) - 1);
                uint32_t hy = (e >> TIE_XY_BITS) & ((1u << TIE_XY_BITS) - 1);
                AuxT<KB, TS> ra = xa[hx], rb = xb[hy];
                bool deep;
                int k = cmp_keys_rec<KB, TS>(ra, rb, deep);
                bool first = k < 0;
                if (k == 0 && !deep) {
                    if constexpr (TS) {
                        first = ra.ts_hi != rb.ts_hi ? ra.ts_hi < rb.ts_hi
                                : ra.ts_lo != rb.ts_lo
                                    ? ra.ts_lo < rb.ts_lo
                                    : a < b;
                    } else {
                        first = cmp_ts_run_blob(R, a, iaS + hx, b,
                                                ibS + hy) < 0;
                    }
                }
                if (!deep)
                    s_list[u] = e | TIE_VALID | (k == 0 ? TIE_KEQ : 0u) |
                                (first ? TIE_AFIRST : 0u);
            }
            __syncthreads();
            /* Each thread takes its own entries back into registers and
             * clears their slots, and only then may any walk store to
             * s_cr. On sorted runs the walks overwrite every staged slot
             * exactly once, so nothing of the list could reach the
             * write-back anyway. On a flagged input (an unsorted run, a
             * corrupt entry's zero prefix) the threads' splits need not
             * fit together and a slot can stay unwritten: it then holds
             * zero, a crossrank that is in range like every other, and
             * not a list entry, whose flag bits would make a rank far
             * past the job's last. */
            #pragma unroll
            for (int m = 0; m < MAXP; m++)
                if (m < (int)ntie) {
                    tie[m] = s_list[lbase + m];
                    s_list[lbase + m] = 0;
                }
            __syncthreads();
        }

        /* The settled entries are hints only: the walk looks a tied pair
         * up among its thread's entries and settles it itself when it is
         * not there (a pair the sweep's provisional "consume both" rule
         * mis-paired, prefix groups wider than 1x1, deep keys), so
         * ordering never depends on the list. */
        if (d < L) {
            for (uint32_t pos = d; pos < dend; pos++) {
                bool take_a;
                bool both = false; /* this step compared (ja, jb) */
                bool keq = false;  /* ... and their keys are equal    */
                if (ja >= lenA)
                    take_a = false;
                else if (jb >= lenB)
                    take_a = true;
                else {
                    both = true;
                    uint64_t pa = sA[ja], pb = sB[jb];
                    if (pa != pb) {
                        take_a = pa < pb;
                    } else {
                        uint32_t h = 0;
                        const uint32_t xy = ja | (jb << TIE_XY_BITS);
                        #pragma unroll
                        for (int m = 0; m < MAXP; m++)
                            if ((tie[m] & TIE_XY_MASK) == xy) h = tie[m];
                        if (h & TIE_VALID) {
                            keq = h & TIE_KEQ;
                            take_a = h & TIE_AFIRST;
                        } else {
                            take_a = tie_eval<KB, TS>(R, aux, a, iaS + ja, b,
                                                      ibS + jb, keq);
                        }
                    }
                }
                /* The entry taken is superseded when the other run's next
                 * entry carries the same key. With both cursors inside the
                 * window that next entry is the one just compared, so the
                 * answer is already known; only a cursor at the window's
                 * end looks past the staged segment. */
                if (take_a) {
                    uint64_t gib = ibS + jb;
                    uint32_t v = (uint32_t)gib;
                    if (both) {
                        if (keq) v |= CR_LOSER;
                    } else if (gib < Nb) {
                        if (gpb[gib] == sA[ja] &&
                            cmp_keys_sfx<KB, TS>(R, aux, a, iaS + ja, b,
                                                 gib) == 0)
                            v |= CR_LOSER;
                    }
                    s_cr[ja] = v;
                    ja++;
                } else {
                    uint64_t gia = iaS + ja;
                    uint32_t v = (uint32_t)gia;
                    if (both) {
                        if (keq) v |= CR_LOSER;
                    } else if (gia < Na) {
                        if (gpa[gia] == sB[jb] &&
                            cmp_keys_sfx<KB, TS>(R, aux, b, ibS + jb, a,
                                                 gia) == 0)
                            v |= CR_LOSER;
                    }
                    s_cr[lenA + jb] = v;
                    jb++;
                }
            }
        }
        __syncthreads();
        /* coalesced writeback of both contiguous output ranges.
         * Crossrank slots are JOB-local (a batched job's runs only pair
         * within their job) */
        {
            uint32_t al = (uint32_t)a - R.job_lo[a];
            uint32_t bl = (uint32_t)b - R.job_lo[b];
            uint32_t sa = bl < al ? bl : bl - 1; /* slot of b in a */
            uint32_t sb = al < bl ? al : al - 1; /* slot of a in b */
            uint32_t* cra = cr + (uint64_t)sa * R.total + R.entry_base[a] +
                            iaS;
            uint32_t* crb = cr + (uint64_t)sb * R.total + R.entry_base[b] +
                            ibS;
            for (uint32_t u = threadIdx.x; u < lenA; u += BLK)
                cra[u] = s_cr[u];
            for (uint32_t u = threadIdx.x; u < lenB; u += BLK)
                crb[u] = s_cr[lenA + u];
        }
        __syncthreads();
    }
}

/* Rank-indexed scratch record: one 16-B scattered write per entry.
 * src packs keep flag (bit 63) | run (bits 48..62) | data offset (48).
 * The survivor scan reads it through a transform iterator. */
struct RankRec {
    uint64_t src;
    uint32_t key_size; /* 8 + key_len (index record field) */
    uint32_t full_size;
};
static_assert(sizeof(RankRec) == 16, "rank record must be 16B");
#define RR_KEEP (1ull << 63)
#define RR_OFF_MASK 0xFFFFFFFFFFFFull

/* The packed survivor sums: bytes in the low 38 bits, count in the high 26
 * (see RankRecPacked below for the bounds that keep them apart). */
#define PK_SHIFT 38
#define PK_MASK ((1ull << PK_SHIFT) - 1)

/* Rank tiles of the survivor-offset stage (further down). */
#define EMIT_BLOCK 256
#define EMIT_ITEMS 8
#define EMIT_TILE (EMIT_BLOCK * EMIT_ITEMS) /* 2048 ranks */

/* Adds each lane's (tile, value) into tile_sum with one atomic per stretch
 * of consecutive lanes that share a tile, never 64 lanes on one address.
 * The lanes of a wave hold consecutive entries of one run (of two at a run
 * seam), whose ranks rise with the lane, so a wave has a handful of
 * stretches. Stretches are told apart by position, not by tile alone, so
 * a tile that comes back after a seam is simply added to twice. Every lane
 * of the wave must call this; lanes without an entry pass v = 0. */
__device__ __forceinline__ void tile_sum_add(uint64_t* tile_sum,
                                             uint64_t tile, uint64_t v) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t prev = __shfl_up(tile, 1);
    uint64_t heads = __ballot(lane == 0 || prev != tile);
    /* the stretch of this lane ends before the next head above it */
    uint64_t above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1);
    uint32_t end =
        above ? (uint32_t)__ffsll((unsigned long long)above) - 1 : 64u;
    #pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        uint64_t dn = __shfl_down(v, o);
        if (lane + o < end) v += dn;
    }
    if (((heads >> lane) & 1) && v)
        atomicAdd((unsigned long long*)(tile_sum + tile),
                  (unsigned long long)v);
}

/* Reduce per-pair crossranks to the global rank, apply the winner /
 * tombstone rules, and emit the rank-indexed scratch records. Also checks
 * each run is strictly sorted by key (flush invariant,
 * lsm_tree.rs:925-946) on the dense pfx/aux arrays. With tile_sum set,
 * every kept entry's packed (count, bytes) contribution is added to the
 * sum of its rank tile, for the tile-wise survivor offsets. The loop is
 * block-uniform, because the wave reduction inside needs every lane. */
template <int KB, bool TS>
__global__ void k_rankreduce(RunsDesc R, const uint64_t* pfx,
                             const AuxT<KB, TS>* aux, const uint32_t* cr,
                             RankRec* rrec, int keep_tombstones,
                             uint32_t* err, uint64_t* tile_sum) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t gb = (uint64_t)blockIdx.x * blockDim.x; gb < R.total;
         gb += stride) {
        uint64_t g = gb + threadIdx.x;
        uint64_t tile = ~0ull, contrib = 0;
        int r = 0;
        uint64_t i = 0;
        EView e;
        bool ok = false;
        if (g < R.total) {
            r = run_of(R, g);
            i = g - R.entry_base[r];
            ok = load_entry(R, r, i, e);
            if (!ok) {
                /* k_prepare has flagged this input; keep memory safe and
                 * park the entry at its local slot (results will be
                 * discarded) */
                RankRec z = {0, 8, 32};
                rrec[g] = z;
            }
        }
        if (ok) {
            if (i + 1 < R.count[r]) {
                uint64_t p0 = pfx[g], p1 = pfx[g + 1];
                if (p0 > p1 ||
                    (p0 == p1 &&
                     cmp_keys_sfx<KB, TS>(R, aux, r, i, r, i + 1) >= 0))
                    atomicOr(err, DERR_UNSORTED);
            }

            /* rank is local to the entry's JOB (independent jobs share one
             * launch); the job's entry base turns it into the global rrec
             * slot, so job outputs concatenate in job order */
            uint64_t rank = i + R.entry_base[R.job_lo[r]];
            bool winner = true;
            int nslots = (int)R.job_hi[r] - (int)R.job_lo[r] - 1;
            for (int s = 0; s < nslots; s++) {
                uint32_t v = cr[(uint64_t)s * R.total + g];
                rank += v & CR_MASK;
                winner &= !(v & CR_LOSER);
            }
            uint64_t dlen = (uint64_t)e.full_size - 32 - e.klen;
            bool keep = winner && (keep_tombstones || dlen != 0);
            RankRec m;
            m.src = ((uint64_t)r << 48) | e.off | (keep ? RR_KEEP : 0);
            m.key_size = e.key_size;
            m.full_size = e.full_size;
            /* rank < total on every valid input; crossranks of a flagged
             * one (results discarded) are not trusted with an address */
            if (rank < R.total) {
                rrec[rank] = m;
                tile = rank / EMIT_TILE;
                if (keep)
                    contrib = (uint64_t)e.full_size | (1ull << PK_SHIFT);
            }
        }
        if (tile_sum) tile_sum_add(tile_sum, tile, contrib);
    }
}

/* transform-iterator functors for the survivor scans (plain arithmetic
 * types + rocprim::plus keep rocPRIM on its decoupled-lookback fast
 * path — a fused custom-STRUCT scan measured 10x slower). When the job
 * fits the packing bounds (bytes < 2^38 = 256 GB, entries < 2^26 = 67M
 * — every BASELINE shape does), ONE u64 scan carries BOTH running sums:
 * survivor bytes in the low 38 bits, survivor count in the high 26
 * (sums stay in-field, so lane-wise u64 addition never carries across);
 * that halves the scan's passes over rrec. Larger jobs fall back to two
 * scans. */
struct RankRecSize {
    __device__ uint64_t operator()(const RankRec& r) const {
        return (r.src & RR_KEEP) ? (uint64_t)r.full_size : 0ull;
    }
};
struct RankRecFlag {
    __device__ uint32_t operator()(const RankRec& r) const {
        return (r.src & RR_KEEP) ? 1u : 0u;
    }
};
struct RankRecPacked {
    __device__ uint64_t operator()(const RankRec& r) const {
        return (r.src & RR_KEEP)
                   ? ((uint64_t)r.full_size | (1ull << PK_SHIFT))
                   : 0ull;
    }
};

/* The two-scan form: survivor byte offsets into dst_off, survivor
 * positions into pos, for n records. rocPRIM's calling convention: with
 * tmp == NULL nothing runs and tmp_bytes receives the scratch size the pair
 * needs; otherwise tmp_bytes is the size of tmp. */
static hipError_t survivor_scans(void* tmp, size_t& tmp_bytes,
                                 const RankRec* rrec, uint64_t* dst_off,
                                 uint32_t* pos, uint64_t n, hipStream_t s) {
    size_t t1 = tmp_bytes, t2 = tmp_bytes;
    hipError_t e = rocprim::exclusive_scan(
        tmp, t1, rocprim::make_transform_iterator(rrec, RankRecSize{}),
        dst_off, (uint64_t)0, n, rocprim::plus<uint64_t>(), s);
    if (e == hipSuccess)
        e = rocprim::exclusive_scan(
            tmp, t2, rocprim::make_transform_iterator(rrec, RankRecFlag{}),
            pos, (uint32_t)0, n, rocprim::plus<uint32_t>(), s);
    if (!tmp) tmp_bytes = t1 > t2 ? t1 : t2;
    return e;
}

/* The step's totals stay on the device: the emit thread that owns the
 * last rank derives them from its scan value and stores them here, and
 * k_winmap / k_copy read them from here, so no host round trip sits
 * between emit and copy. On a flagged input (d_err set; prepare and
 * rank-reduce are complete in stream order) the totals are zero, so a
 * corrupt index can never drive the copy. The host reads the record once,
 * after the copy. */
struct StepTotals {
    uint64_t total_out; /* output data bytes */
    uint64_t n_surv;    /* surviving entries */
    uint64_t err;       /* d_err[0] as the emit kernel saw it */
};

__device__ __forceinline__ void store_totals(StepTotals* tot,
                                             const uint32_t* err,
                                             const RankRec& last,
                                             uint64_t last_off,
                                             uint64_t last_pos) {
    uint32_t e = *err;
    uint64_t kept = (last.src & RR_KEEP) ? 1 : 0;
    tot->total_out = e ? 0 : last_off + (kept ? last.full_size : 0);
    tot->n_surv = e ? 0 : last_pos + kept;
    tot->err = e;
}

/* Output index records are the input format: offset u64 | key_size u32 |
 * full_size u32 (entry_writer.rs:79-87, offsets recomputed from 0).
 * src_map gets the ABSOLUTE device address of each survivor's bytes. */
__global__ void k_emit(RunsDesc R, const RankRec* rrec,
                       const uint64_t* dst_off, const uint32_t* pos,
                       uint64_t total, uint8_t* out_index,
                       uint64_t* src_map, const uint32_t* err,
                       StepTotals* tot) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         g < total; g += stride) {
        RankRec m = rrec[g];
        if (g + 1 == total)
            store_totals(tot, err, m, dst_off[g], pos[g]);
        if (!(m.src & RR_KEEP)) continue;
        uint64_t p = pos[g];
        uint8_t* rec = out_index + p * 16;
        uint64_t off = dst_off[g];
        __builtin_memcpy(rec, &off, 8);
        __builtin_memcpy(rec + 8, &m.key_size, 4);
        __builtin_memcpy(rec + 12, &m.full_size, 4);
        src_map[p] = (uint64_t)(R.data[(m.src >> 48) & 0x7FFF] +
                                (m.src & RR_OFF_MASK));
    }
}

/* k_emit for the packed single-scan mode: offsets and positions decode
 * from one u64 (low 38 bits = byte offset, high 26 = survivor index). */
__global__ void k_emit_packed(RunsDesc R, const RankRec* rrec,
                              const uint64_t* packed, uint64_t total,
                              uint8_t* out_index, uint64_t* src_map,
                              const uint32_t* err, StepTotals* tot) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         g < total; g += stride) {
        RankRec m = rrec[g];
        if (g + 1 == total)
            store_totals(tot, err, m, packed[g] & PK_MASK,
                         packed[g] >> PK_SHIFT);
        if (!(m.src & RR_KEEP)) continue;
        uint64_t v = packed[g];
        uint64_t p = v >> PK_SHIFT;
        uint8_t* rec = out_index + p * 16;
        uint64_t off = v & PK_MASK;
        __builtin_memcpy(rec, &off, 8);
        __builtin_memcpy(rec + 8, &m.key_size, 4);
        __builtin_memcpy(rec + 12, &m.full_size, 4);
        src_map[p] = (uint64_t)(R.data[(m.src >> 48) & 0x7FFF] +
                                (m.src & RR_OFF_MASK));
    }
}

/* ------------------------------------------------------------------ */
/* Survivor offsets by rank tile (packed mode of the job path)         */
/*                                                                     */
/* A tile is EMIT_TILE consecutive ranks. k_rankreduce, which knows    */
/* every entry's keep flag and size when it writes the rank record,    */
/* adds the entry's packed contribution (RankRecPacked) to its tile's  */
/* sum; k_tilebase turns the few thousand sums into exclusive bases;   */
/* k_emit_tile scans its own tile from that base and writes what       */
/* k_emit_packed writes. The rank records are read once, and no        */
/* per-entry offset array exists. Sums of packed values stay in-field  */
/* for the reason given above RankRecPacked, in any order of addition. */
/* ------------------------------------------------------------------ */
__device__ __forceinline__ uint64_t packed_contrib(const RankRec& r) {
    return RankRecPacked{}(r);
}

/* s_v slot of tile-local rank i: one pad word per EMIT_ITEMS, so that
 * both the rank-per-lane and the EMIT_ITEMS-per-lane access patterns
 * spread over the LDS banks */
__device__ __forceinline__ uint32_t emit_slot(uint32_t i) {
    return i + i / EMIT_ITEMS;
}

/* Exclusive scan of the tile sums, in place: one block, 1024 sums per
 * round, the running total carried from round to round. No block waits
 * for another. */
#define TILEBASE_BLOCK 1024
__global__ __launch_bounds__(TILEBASE_BLOCK) void k_tilebase(
    uint64_t* tile_sum, uint32_t n_tiles) {
    __shared__ uint64_t s_w[TILEBASE_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += TILEBASE_BLOCK) {
        uint32_t t = t0 + threadIdx.x;
        uint64_t v = t < n_tiles ? tile_sum[t] : 0ull;
        uint64_t incl = v;
        #pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            uint64_t up = __shfl_up(incl, o);
            if (lane >= (uint32_t)o) incl += up;
        }
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        uint64_t before = 0, all = 0;
        #pragma unroll
        for (int w = 0; w < TILEBASE_BLOCK / 64; w++) {
            uint64_t wt = s_w[w];
            if ((uint32_t)w < wave) before += wt;
            all += wt;
        }
        if (t < n_tiles) tile_sum[t] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
}

/* One block per tile. The tile's rank records are loaded coalesced (item k
 * of thread t is rank k * EMIT_BLOCK + t of the tile); their packed
 * contributions go through LDS so that each thread scans EMIT_ITEMS
 * consecutive ranks, and come back as exclusive (position, offset) values
 * for the records the threads still hold. Writes what k_emit_packed
 * writes. With win_shift != 0 (copy windows of 1 << win_shift bytes,
 * win_cap slots in win_p0) it also fills the copy's window map: the
 * survivor whose bytes cover a window start is the window's first one, and
 * a survivor no larger than a window covers at most one start. A larger
 * one sets *need_winmap instead, and k_winmap fills the map as before. */
__global__ __launch_bounds__(EMIT_BLOCK) void k_emit_tile(
    RunsDesc R, const RankRec* rrec, const uint64_t* tile_base,
    uint64_t total, uint8_t* out_index, uint64_t* src_map,
    const uint32_t* err, StepTotals* tot, uint32_t win_shift,
    uint64_t win_cap, uint32_t* win_p0, uint32_t* need_winmap) {
    __shared__ uint64_t s_v[EMIT_TILE + EMIT_TILE / EMIT_ITEMS];
    __shared__ uint64_t s_w[EMIT_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t n_tiles = (total + EMIT_TILE - 1) / EMIT_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t g0 = tile * EMIT_TILE;
        uint64_t src[EMIT_ITEMS];
        uint32_t ksz[EMIT_ITEMS], fsz[EMIT_ITEMS];
        #pragma unroll
        for (int k = 0; k < EMIT_ITEMS; k++) {
            uint64_t g = g0 + (uint32_t)k * EMIT_BLOCK + threadIdx.x;
            src[k] = 0, ksz[k] = 0, fsz[k] = 0;
            if (g < total) {
                RankRec m = rrec[g];
                src[k] = m.src, ksz[k] = m.key_size, fsz[k] = m.full_size;
            }
            s_v[emit_slot(k * EMIT_BLOCK + threadIdx.x)] =
                (src[k] & RR_KEEP) ? ((uint64_t)fsz[k] | (1ull << PK_SHIFT))
                                   : 0ull;
        }
        __syncthreads();
        uint64_t loc[EMIT_ITEMS], sum = 0;
        #pragma unroll
        for (int k = 0; k < EMIT_ITEMS; k++) {
            loc[k] = sum; /* exclusive within the thread */
            sum += s_v[emit_slot(threadIdx.x * EMIT_ITEMS + k)];
        }
        uint64_t incl = sum;
        #pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            uint64_t up = __shfl_up(incl, o);
            if (lane >= (uint32_t)o) incl += up;
        }
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        uint64_t base = tile_base[tile] + incl - sum;
        #pragma unroll
        for (int w = 0; w < EMIT_BLOCK / 64; w++)
            if ((uint32_t)w < wave) base += s_w[w];
        /* a thread rewrites only the slots it has just read */
        #pragma unroll
        for (int k = 0; k < EMIT_ITEMS; k++)
            s_v[emit_slot(threadIdx.x * EMIT_ITEMS + k)] = base + loc[k];
        __syncthreads();
        #pragma unroll
        for (int k = 0; k < EMIT_ITEMS; k++) {
            uint64_t g = g0 + (uint32_t)k * EMIT_BLOCK + threadIdx.x;
            if (g >= total) continue;
            uint64_t v = s_v[emit_slot(k * EMIT_BLOCK + threadIdx.x)];
            uint64_t p = v >> PK_SHIFT, off = v & PK_MASK;
            const uint32_t key_size = ksz[k], full_size = fsz[k];
            if (g + 1 == total) {
                RankRec last = {src[k], key_size, full_size};
                store_totals(tot, err, last, off, p);
            }
            /* p < total always holds on valid input; on a flagged one
             * (totals zero, nothing copied) the sizes may not add up */
            if (!(src[k] & RR_KEEP) || p >= total) continue;
            uint8_t* rec = out_index + p * 16;
            __builtin_memcpy(rec, &off, 8);
            __builtin_memcpy(rec + 8, &key_size, 4);
            __builtin_memcpy(rec + 12, &full_size, 4);
            src_map[p] = (uint64_t)(R.data[(src[k] >> 48) & 0x7FFF] +
                                    (src[k] & RR_OFF_MASK));
            if (win_shift) {
                if (full_size <= (1u << win_shift)) {
                    /* the first window start at or after off */
                    uint64_t w = (off + (1u << win_shift) - 1) >> win_shift;
                    if ((w << win_shift) < off + full_size && w < win_cap)
                        win_p0[w] = (uint32_t)p;
                } else {
                    *need_winmap = 1;
                }
            }
        }
        __syncthreads(); /* s_v and s_w are reused by the next tile */
    }
}

/* The packed scan value at rank g (exclusive), rebuilt from the tile bases
 * where no per-entry array holds it: one block sums the contributions of
 * the ranks of g's tile below g. Used for the few job boundaries a batched
 * job's result is sliced at, after the step. */
__global__ __launch_bounds__(EMIT_BLOCK) void k_tile_value_at(
    const RankRec* rrec, const uint64_t* tile_base, uint64_t g,
    uint64_t* out) {
    __shared__ uint64_t s_w[EMIT_BLOCK / 64];
    const uint64_t g0 = g / EMIT_TILE * EMIT_TILE;
    uint64_t v = 0;
    for (uint64_t i = g0 + threadIdx.x; i < g; i += EMIT_BLOCK)
        v += packed_contrib(rrec[i]);
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t s = tile_base[g / EMIT_TILE];
        for (int w = 0; w < EMIT_BLOCK / 64; w++) s += s_w[w];
        *out = s;
    }
}

/* Balanced verbatim copy: a 16-KiB destination window per 256-thread
 * block, 4 x 16-B granules per thread (independent loads/stores for ILP;
 * granule passes are thread-contiguous so stores coalesce). Entries are
 * >= 32 B (validated), so a window intersects < 16384/32 + 2 entries and
 * SPAN=516 staged offsets always cover it; a 16-B granule straddles at
 * most one entry boundary. */
#define COPY_BLOCK 256
#define COPY_WINDOW 16384
#define COPY_SPAN 516

#define COPY_GRANULES (COPY_WINDOW / 16)
/* geometry variants for within-probe A/B (env DBEEL_COPY_VARIANT):
 * 0 = 256 threads x 16 KiB (default), 1 = 256 x 8 KiB,
 * 2 = 512 x 16 KiB, 3 = 512 x 32 KiB */

/* Per destination window, the largest survivor p with offset(p) <= window
 * start — one thread per window (parallel), consumed by k_copy. With
 * `need` set and clear, the map is already there and nothing runs. */
__global__ void k_winmap(const uint8_t* out_index, const StepTotals* tot,
                         uint32_t win, uint32_t* win_p0,
                         const uint32_t* need) {
    if (need && !*need) return;
    const uint64_t n_surv = tot->n_surv, total_bytes = tot->total_out;
    uint64_t n_windows = (total_bytes + win - 1) / win;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         w < n_windows; w += stride) {
        uint64_t wstart = (uint64_t)w * win;
        uint64_t lo = 0, hi = n_surv; /* first offset > wstart, minus 1 */
        while (lo < hi) {
            uint64_t mid = (lo + hi) >> 1;
            if (ld_u64(out_index + mid * 16) <= wstart)
                lo = mid + 1;
            else
                hi = mid;
        }
        win_p0[w] = (uint32_t)(lo - 1); /* offset(0)=0 -> lo >= 1 */
    }
}

template <int BLK, int WIN>
__global__ __launch_bounds__(BLK) void k_copy(
    const uint8_t* out_index, const uint64_t* src_map,
    const uint32_t* win_p0, const StepTotals* tot, uint8_t* out_data) {
    /* the grid is sized from an upper bound on the output; blocks whose
     * first window lies past the real end fall straight through */
    const uint64_t n_surv = tot->n_surv, total_bytes = tot->total_out;
    constexpr int SPAN = WIN / 32 + 4;
    constexpr int GRAN = WIN / 16;
    __shared__ uint64_t s_off[SPAN + 1];
    __shared__ uint64_t s_src[SPAN];
    __shared__ uint16_t s_gid[GRAN]; /* granule -> entry slot */

    uint64_t n_windows = (total_bytes + WIN - 1) / WIN;
    for (uint64_t w = blockIdx.x; w < n_windows; w += gridDim.x) {
        uint64_t wstart = w * WIN;
        uint64_t p0 = win_p0[w];
        /* entries intersecting this window are p0 .. win_p0[w+1]; staging
         * only those (not the worst-case SPAN) saves ~30x index re-reads
         * on KiB-sized entries */
        uint64_t p_end = (w + 1 < n_windows) ? (uint64_t)win_p0[w + 1] + 1
                                             : n_surv;
        uint32_t cnt = (uint32_t)(p_end - p0);
        if (cnt > SPAN) cnt = SPAN;
        if (cnt > n_surv - p0) cnt = (uint32_t)(n_surv - p0);
        for (uint32_t u = threadIdx.x; u <= cnt; u += BLK) {
            uint64_t p = p0 + u;
            if (u == cnt)
                s_off[cnt] = (p < n_surv) ? ld_u64(out_index + p * 16)
                                          : total_bytes;
            else {
                s_off[u] = ld_u64(out_index + p * 16);
                s_src[u] = src_map[p];
            }
        }
        __syncthreads();
        /* fill the granule -> entry map: entry slot u owns granules whose
         * START byte lies in [s_off[u], s_off[u+1]). Two fills: an
         * entry-sweep when entries are small (each writes few granules),
         * a granule-parallel binary search when few LARGE entries cover
         * the window (the sweep would serialize hundreds of LDS writes
         * on a handful of threads — measured 2x on 4 KiB values). */
        if (cnt >= 128) {
            for (uint32_t u = threadIdx.x; u < cnt; u += BLK) {
                uint64_t b0 = s_off[u], b1 = s_off[u + 1];
                uint64_t g0 = (b0 <= wstart) ? 0 : ((b0 - wstart + 15) >> 4);
                uint64_t g1 = (b1 - wstart + 15) >> 4; /* exclusive */
                if (g1 > GRAN) g1 = GRAN;
                for (uint64_t g = g0; g < g1; g++) s_gid[g] = (uint16_t)u;
            }
        } else {
            #pragma unroll
            for (int q = 0; q < GRAN / BLK; q++) {
                uint32_t g = q * BLK + threadIdx.x;
                uint64_t gpos = wstart + (uint64_t)g * 16;
                uint32_t lo = 0, hi = cnt; /* largest u: s_off[u] <= gpos */
                while (lo < hi) {
                    uint32_t mid = (lo + hi) >> 1;
                    if (s_off[mid] <= gpos)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                s_gid[g] = (uint16_t)(lo ? lo - 1 : 0);
            }
        }
        __syncthreads();

        typedef unsigned int v4u __attribute__((ext_vector_type(4)));
        if (wstart + WIN <= total_bytes) {
            /* full interior window: every granule is a whole 16 B. Two
             * phases — gather all GRAN/BLK granule values into registers
             * first (independent load chains, keeps several loads in
             * flight per wave), then store. The single-phase form left
             * most waves parked on one load at a time (93% parked on the
             * 4 KiB-value shape, r01 profile). */
            v4u vv[GRAN / BLK];
            #pragma unroll
            for (int q = 0; q < GRAN / BLK; q++) {
                uint32_t gl = q * BLK + threadIdx.x; /* window-local */
                uint64_t gpos = wstart + (uint64_t)gl * 16;
                uint32_t j = s_gid[gl];
                uint64_t e_end = s_off[j + 1];
                const uint8_t* src = (const uint8_t*)s_src[j] +
                                     (gpos - s_off[j]);
                if (gpos + 16 <= e_end) {
                    /* plain (cached) loads: a nontemporal-load variant
                     * measured 15-18% SLOWER (copy 2.15 -> 2.52 ms on
                     * cfg3) — adjacent granules of the same entry share
                     * lines through L2 and NT hints forfeit that */
                    __builtin_memcpy(&vv[q], src, 16);
                } else {
                    /* one entry boundary inside the granule: 16-B blend
                     * of the entry tail and the next survivor's head.
                     * Byte loops here cost a whole wave ~3k serial
                     * cycles, and odd entry sizes put one straddle in
                     * nearly every wave (measured 2.4x on odd-size
                     * values). Reading past either entry stays inside
                     * the padded input slab. */
                    uint32_t c1 = (uint32_t)(e_end - gpos); /* 1..15 */
                    const uint8_t* src2 = (const uint8_t*)s_src[j + 1];
                    uint64_t l0, h0, l2, h2;
                    __builtin_memcpy(&l0, src, 8);
                    __builtin_memcpy(&h0, src + 8, 8);
                    __builtin_memcpy(&l2, src2, 8);
                    __builtin_memcpy(&h2, src2 + 8, 8);
                    uint64_t lo, hi;
                    if (c1 < 8) {
                        uint32_t sh = 8 * c1;
                        uint64_t m = (~0ull) >> (64 - sh);
                        lo = (l0 & m) | (l2 << sh);
                        hi = (h2 << sh) | (l2 >> (64 - sh));
                    } else {
                        uint32_t c = c1 - 8; /* 0..7 */
                        lo = l0;
                        if (c == 0) {
                            hi = l2;
                        } else {
                            uint64_t m = (~0ull) >> (64 - 8 * c);
                            hi = (h0 & m) | (l2 << (8 * c));
                        }
                    }
                    __builtin_memcpy(&vv[q], &lo, 8);
                    __builtin_memcpy(
                        reinterpret_cast<uint8_t*>(&vv[q]) + 8, &hi, 8);
                }
            }
            /* streamed once, never re-read: keep L2 for sources */
            #pragma unroll
            for (int q = 0; q < GRAN / BLK; q++) {
                uint32_t gl = q * BLK + threadIdx.x;
                __builtin_nontemporal_store(
                    vv[q], reinterpret_cast<v4u*>(out_data + wstart +
                                                  (uint64_t)gl * 16));
            }
        } else {
            /* the job's final (partial) window */
            #pragma unroll
            for (int q = 0; q < GRAN / BLK; q++) {
                uint32_t gl = q * BLK + threadIdx.x;
                uint64_t gpos = wstart + (uint64_t)gl * 16;
                if (gpos >= total_bytes) break;
                uint32_t j = s_gid[gl];
                uint64_t e_end = s_off[j + 1];
                const uint8_t* src = (const uint8_t*)s_src[j] +
                                     (gpos - s_off[j]);
                uint32_t nbytes = (uint32_t)(
                    (total_bytes - gpos) < 16 ? (total_bytes - gpos) : 16);
                uint8_t* dst = out_data + gpos;
                uint32_t c1 = (uint32_t)(gpos + nbytes <= e_end
                                             ? nbytes
                                             : e_end - gpos);
                for (uint32_t b = 0; b < c1; b++) dst[b] = src[b];
                if (c1 < nbytes) {
                    const uint8_t* src2 = (const uint8_t*)s_src[j + 1];
                    for (uint32_t b = c1; b < nbytes; b++)
                        dst[b] = src2[b - c1];
                }
            }
        }
        __syncthreads();
    }
}

/* ------------------------------------------------------------------ */
/* Run encoder (the memtable-flush path)                              */
/*                                                                    */
/* Encodes an already-sorted (key, value, timestamp) stream into a    */
/* run: the same bincode-fixint entry layout + 16-B index records as  */
/* flush_memtable_to_disk / EntryWriter (lsm_tree.rs:925-946,         */
/* entry_writer.rs:71-98). Wave-per-entry copy: lanes move 8-byte     */
/* chunks of key/value bytes; the header fields and timestamp are     */
/* written by lane 0.                                                 */
/* ------------------------------------------------------------------ */

__global__ void k_encode_sizes(uint64_t n, const uint64_t* key_off,
                               const uint64_t* val_off, uint64_t* sizes) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += stride) {
        sizes[i] = 32 + (key_off[i + 1] - key_off[i]) +
                   (val_off[i + 1] - val_off[i]);
    }
}

__global__ void k_encode_index(uint64_t n, const uint64_t* key_off,
                               const uint64_t* dst_off,
                               const uint64_t* sizes, uint8_t* out_index) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += stride) {
        uint8_t* rec = out_index + i * 16;
        uint64_t off = dst_off[i];
        uint32_t key_size = (uint32_t)(8 + key_off[i + 1] - key_off[i]);
        uint32_t full_size = (uint32_t)sizes[i];
        __builtin_memcpy(rec, &off, 8);
        __builtin_memcpy(rec + 8, &key_size, 4);
        __builtin_memcpy(rec + 12, &full_size, 4);
    }
}

__device__ __forceinline__ void wave_copy_bytes(uint8_t* dst,
                                                const uint8_t* src,
                                                uint64_t n, uint32_t lane) {
    /* 8-byte chunks per lane, byte tail by lane 0 */
    uint64_t chunks = n >> 3;
    for (uint64_t c = lane; c < chunks; c += 64) {
        uint64_t v;
        __builtin_memcpy(&v, src + c * 8, 8);
        __builtin_memcpy(dst + c * 8, &v, 8);
    }
    if (lane == 0)
        for (uint64_t b = chunks * 8; b < n; b++) dst[b] = src[b];
}

__global__ void k_encode_data(uint64_t n, const uint8_t* keys,
                              const uint64_t* key_off, const uint8_t* vals,
                              const uint64_t* val_off, const uint8_t* ts,
                              const uint64_t* dst_off, uint8_t* out_data) {
    uint32_t lane = threadIdx.x & 63;
    uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t i = wave; i < n; i += n_waves) {
        uint64_t klen = key_off[i + 1] - key_off[i];
        uint64_t vlen = val_off[i + 1] - val_off[i];
        uint8_t* dst = out_data + dst_off[i];
        if (lane == 0) {
            __builtin_memcpy(dst, &klen, 8);
            __builtin_memcpy(dst + 8 + klen, &vlen, 8);
            __builtin_memcpy(dst + 16 + klen + vlen, ts + i * 16, 16);
        }
        wave_copy_bytes(dst + 8, keys + key_off[i], klen, lane);
        wave_copy_bytes(dst + 16 + klen, vals + val_off[i], vlen, lane);
    }
}

extern "C" int dbeel_gpu_encode_run(uint64_t n_entries, const uint8_t* keys,
                                    const uint64_t* key_offsets,
                                    const uint8_t* values,
                                    const uint64_t* value_offsets,
                                    const uint8_t* timestamps, int device,
                                    dbeel_compact_result* out) {
    g_err[0] = 0;
    if (!out || (n_entries && (!keys || !key_offsets || !values ||
                               !value_offsets || !timestamps))) {
        set_err("encode_run: null argument");
        return DBEEL_ERR_INVALID_ARG;
    }
    memset(out, 0, sizeof *out);
    int rc = select_device(device);
    if (rc) return rc;
    if (n_entries == 0) {
        out->data = (uint8_t*)malloc(1);
        out->index = (uint8_t*)malloc(1);
        return DBEEL_OK;
    }
    uint64_t n = n_entries;
    uint64_t kbytes = key_offsets[n], vbytes = value_offsets[n];
    for (uint64_t i = 0; i < n; i++) {
        uint64_t klen = key_offsets[i + 1] - key_offsets[i];
        uint64_t vlen = value_offsets[i + 1] - value_offsets[i];
        if (key_offsets[i + 1] < key_offsets[i] ||
            value_offsets[i + 1] < value_offsets[i] ||
            32 + klen + vlen > 0xFFFFFFFFull) {
            set_err("entry %llu too large or offsets not monotone",
                    (unsigned long long)i);
            return DBEEL_ERR_ITEM_TOO_LARGE; /* error.rs:60-61 analogue */
        }
    }

    uint8_t *d_keys = nullptr, *d_vals = nullptr, *d_ts = nullptr,
            *d_outd = nullptr, *d_outi = nullptr;
    uint64_t *d_koff = nullptr, *d_voff = nullptr, *d_sizes = nullptr,
             *d_doff = nullptr;
    void* d_tmp = nullptr;
    hipStream_t s = nullptr;
    size_t tmp_bytes = 0;
    /* guards run in reverse: the device side is released (hipFree waits
     * for the stream) before a failed call's host buffers go */
    ScopeGuard drop_out([&] { dbeel_gpu_result_free(out); });
    ScopeGuard release([&] {
        hipFree(d_keys);
        hipFree(d_vals);
        hipFree(d_ts);
        hipFree(d_koff);
        hipFree(d_voff);
        hipFree(d_sizes);
        hipFree(d_doff);
        hipFree(d_tmp);
        hipFree(d_outd);
        hipFree(d_outi);
        if (s) hipStreamDestroy(s);
    });

    HIP_CHECK(hipStreamCreate(&s));
    HIP_CHECK(hipMalloc(&d_keys, kbytes ? kbytes : 1));
    HIP_CHECK(hipMalloc(&d_vals, vbytes ? vbytes : 1));
    HIP_CHECK(hipMalloc(&d_ts, n * 16));
    HIP_CHECK(hipMalloc(&d_koff, (n + 1) * 8));
    HIP_CHECK(hipMalloc(&d_voff, (n + 1) * 8));
    HIP_CHECK(hipMalloc(&d_sizes, n * 8));
    HIP_CHECK(hipMalloc(&d_doff, n * 8));
    HIP_CHECK(hipMemcpyAsync(d_keys, keys, kbytes ? kbytes : 1,
                             hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_vals, values, vbytes ? vbytes : 1,
                             hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_ts, timestamps, n * 16,
                             hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_koff, key_offsets, (n + 1) * 8,
                             hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_voff, value_offsets, (n + 1) * 8,
                             hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_encode_sizes, dim3(pick_grid(n, 256)), dim3(256), 0,
                       s, n, d_koff, d_voff, d_sizes);
    HIP_CHECK(rocprim::exclusive_scan(nullptr, tmp_bytes, d_sizes, d_doff,
                                      (uint64_t)0, n,
                                      rocprim::plus<uint64_t>(), s));
    HIP_CHECK(hipMalloc(&d_tmp, tmp_bytes));
    HIP_CHECK(rocprim::exclusive_scan(d_tmp, tmp_bytes, d_sizes, d_doff,
                                      (uint64_t)0, n,
                                      rocprim::plus<uint64_t>(), s));
    const uint64_t total = 32 * n + kbytes + vbytes; /* 32+klen+vlen each */
    HIP_CHECK(hipMalloc(&d_outd, total));
    HIP_CHECK(hipMalloc(&d_outi, n * 16));
    hipLaunchKernelGGL(k_encode_index, dim3(pick_grid(n, 256)), dim3(256), 0,
                       s, n, d_koff, d_doff, d_sizes, d_outi);
    hipLaunchKernelGGL(k_encode_data, dim3(pick_grid(n * 64, 256)), dim3(256),
                       0, s, n, d_keys, d_koff, d_vals, d_voff, d_ts, d_doff,
                       d_outd);
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());

    out->data = (uint8_t*)malloc(total ? total : 1);
    out->index = (uint8_t*)malloc(n * 16);
    if (!out->data || !out->index) {
        set_err("host malloc failed");
        return DBEEL_ERR_OOM;
    }
    HIP_CHECK(hipMemcpyAsync(out->data, d_outd, total,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(out->index, d_outi, n * 16,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    out->data_len = total;
    out->index_len = n * 16;
    out->entries_written = n;
    drop_out.dismiss();
    return DBEEL_OK;
}

/* ------------------------------------------------------------------ */
/* Host side                                                          */
/* ------------------------------------------------------------------ */

static inline uint64_t ld_u64_host(const uint8_t* p) {
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}

/* Max key_size across all uploaded index slabs — picks the aux tier. */
__global__ void k_maxks(RunsDesc R, uint32_t* out) {
    __shared__ uint32_t smax;
    if (threadIdx.x == 0) smax = 0;
    __syncthreads();
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t m = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         g < R.total; g += stride) {
        int r = run_of(R, g);
        uint64_t i = g - R.entry_base[r];
        uint32_t ks = ld_u32(R.index[r] + i * 16 + 8);
        if (ks > m) m = ks;
    }
    atomicMax(&smax, m);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(out, smax);
}

/* Adds delta (mod 2^64) to the offset field of n index records, in place:
 * one 8-byte load and one 8-byte store per record, the other 8 bytes of the
 * record untouched. Serves both directions of a sliced compaction: -off_lo
 * on a slice's uploaded input records, +base on output records about to
 * leave. The records need no alignment (an input index follows its run's
 * data bytes in the slab). */
__global__ void k_index_rebase(uint8_t* index, uint64_t n, uint64_t delta) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        uint8_t* rec = index + i * 16;
        uint64_t off = ld_u64(rec) + delta;
        __builtin_memcpy(rec, &off, 8);
    }
}

struct dbeel_gpu_job {
    int device = -1;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr; /* streamed-ingest H2D lane */
    hipEvent_t ev[8] = {};
    int prep_valid = 0; /* set by job_ingest: pfx/aux/d_err already built
                           for the current inputs (overlapped with the
                           transfer); job_run skips the prepare stage.
                           job_create leaves it 0 so the resident
                           measurement mode always runs the full
                           pipeline per step. */
    RunsDesc desc{};
    uint8_t* d_input = nullptr; /* one slab: all run data+index            */
    bool borrowed = false;      /* desc points at device memory owned by a
                                   resident reader: no slab, never freed
                                   here, ingest refused                    */
    RankRec* d_rank = nullptr;
    uint64_t* d_dstoff = nullptr;
    uint32_t* d_pos = nullptr;
    int aux_kind = 2;           /* 0: 16-B, 1: 32-B, 2: 64-B aux records   */
    uint8_t* d_outindex = nullptr;
    uint64_t* d_srcmap = nullptr;
    uint8_t* d_outdata = nullptr;
    void* d_scantmp = nullptr;
    size_t scantmp_bytes = 0;
    uint32_t* d_err = nullptr;   /* one allocation, zeroed per step: the
                                    error words (2 x u32), the flag that
                                    asks for k_winmap (u32, + pad), then
                                    the rank-tile sums                  */
    uint32_t* d_needwin = nullptr; /* = d_err + 2                       */
    uint64_t* d_tilesum = nullptr; /* = d_err + 4: n_tiles packed sums,
                                      exclusive bases after k_tilebase  */
    uint32_t n_tiles = 0;
    uint64_t* d_pfx = nullptr;   /* dense big-endian key prefixes       */
    void* d_aux = nullptr;       /* dense 64B search records            */
    uint32_t* d_cr = nullptr;    /* per-pair crossranks, column-major   */
    void* d_pairs = nullptr;     /* PairDesc table                      */
    uint32_t n_pairs = 0;
    uint64_t total_chunks = 0;
    uint32_t* d_winp0 = nullptr; /* copy window -> first survivor       */
    uint64_t* d_corners = nullptr; /* corank chunk start corners        */
    StepTotals* d_tot = nullptr; /* step totals, written by emit         */
    StepTotals* h_tot = nullptr; /* pinned: the one read per step        */
    uint64_t total_entries = 0;
    uint64_t total_data_bytes = 0;
    uint64_t input_bytes = 0;
    std::vector<uint64_t> job_gbase; /* entry base per job (+ total) */
    /* last-run results */
    int last_scan_packed = 0; /* 1: d_dstoff holds packed (pos<<38|off);
                                 2: tile mode, no per-entry array: the
                                 same packed value is rebuilt on demand
                                 from d_tilesum and d_rank */
    uint64_t out_data_len = 0;
    uint64_t out_entries = 0;
    bool have_result = false;
    double h2d_ms = 0.0;
};

static int validate_runs(const dbeel_run_view* runs, size_t n_runs) {
    if (!runs || n_runs == 0) {
        set_err("runs is null or empty");
        return DBEEL_ERR_INVALID_ARG;
    }
    if (n_runs > MAX_RUNS) {
        set_err("n_runs %zu exceeds MAX_RUNS %d", n_runs, MAX_RUNS);
        return DBEEL_ERR_INVALID_ARG;
    }
    for (size_t r = 0; r < n_runs; r++) {
        if (runs[r].index_len % 16) {
            set_err("run %zu: index_len %zu not a multiple of 16", r,
                    runs[r].index_len);
            return DBEEL_ERR_CORRUPT;
        }
        if ((runs[r].data_len && !runs[r].data) ||
            (runs[r].index_len && !runs[r].index)) {
            set_err("run %zu: null pointer with nonzero length", r);
            return DBEEL_ERR_INVALID_ARG;
        }
        if (runs[r].data_len >= (1ull << 48)) {
            set_err("run %zu: data_len too large", r);
            return DBEEL_ERR_ITEM_TOO_LARGE;
        }
        if (runs[r].index_len / 16 >= (1ull << 31)) {
            /* crossranks carry a 31-bit payload (CR_LOSER uses bit 31):
             * enforce the representation bound explicitly rather than by
             * incidental OOM */
            set_err("run %zu: 2^31 or more entries unsupported", r);
            return DBEEL_ERR_ITEM_TOO_LARGE;
        }
    }
    uint64_t total = 0;
    for (size_t r = 0; r < n_runs; r++) total += runs[r].index_len / 16;
    if (total >= (1ull << 32)) {
        /* survivor positions (d_pos scan, win_p0) are uint32 */
        set_err("job has 2^32 or more total entries");
        return DBEEL_ERR_ITEM_TOO_LARGE;
    }
    return DBEEL_OK;
}

/* borrowed: runs[].data / .index are DEVICE pointers on `device` that
 * stay valid (and padded like a slab) for the job's lifetime; nothing is
 * uploaded. Nothing in the pipeline needs one contiguous slab: k_emit
 * stores absolute source addresses, the pair table and the aux tier
 * depend only on counts and key sizes.
 *
 * off_bias (may be NULL; not with borrowed): off_bias[r] is subtracted on
 * the device from every index record offset of run r right after its index
 * upload, before anything reads the records — the run view is a slice of a
 * larger run whose records still carry offsets into the whole. A record
 * that lies below the bias wraps to a huge offset, which load_entry's
 * wrap-proof bounds test rejects (DBEEL_ERR_CORRUPT from job_run): that
 * test is relied on, there is no second one. */
static int job_create_impl(const dbeel_run_view* runs, size_t n_runs,
                           const uint32_t* runs_per_job, size_t n_jobs,
                           int device, dbeel_gpu_job** out_job,
                           bool borrowed = false,
                           const uint64_t* off_bias = nullptr) {
    g_err[0] = 0;
    if (!out_job) {
        set_err("out_job is null");
        return DBEEL_ERR_INVALID_ARG;
    }
    *out_job = nullptr;
    int rc = validate_runs(runs, n_runs);
    if (rc) return rc;
    {
        uint64_t sum = 0;
        for (size_t j = 0; j < n_jobs; j++) {
            if (!runs_per_job[j]) {
                set_err("job %zu has zero runs", j);
                return DBEEL_ERR_INVALID_ARG;
            }
            sum += runs_per_job[j];
        }
        if (sum != n_runs) {
            set_err("runs_per_job sums to %llu != n_runs %zu",
                    (unsigned long long)sum, n_runs);
            return DBEEL_ERR_INVALID_ARG;
        }
    }
    rc = select_device(device);
    if (rc) return rc;

    dbeel_gpu_job* job = new (std::nothrow) dbeel_gpu_job();
    if (!job) return DBEEL_ERR_OOM;
    ScopeGuard drop_job([&] { dbeel_gpu_job_destroy(job); });
    job->device = device;
    job->borrowed = borrowed;

    uint64_t input_bytes = 0, total = 0, total_data = 0;
    for (size_t r = 0; r < n_runs; r++) {
        input_bytes += runs[r].data_len + runs[r].index_len;
        total += runs[r].index_len / 16;
        total_data += runs[r].data_len;
    }
    job->total_entries = total;
    job->total_data_bytes = total_data;
    job->input_bytes = input_bytes;

    HIP_CHECK(hipStreamCreate(&job->stream));
    for (int i = 0; i < 8; i++) HIP_CHECK(hipEventCreate(&job->ev[i]));

    /* +-16 B padding: the copy kernel's aligned-base loads may touch up
     * to 15 B before/after an entry's bytes */
    if (!borrowed)
        HIP_CHECK(hipMalloc(&job->d_input,
                            (input_bytes ? input_bytes : 16) + 32));
    uint64_t n = total ? total : 1;
    HIP_CHECK(hipMalloc(&job->d_rank, n * sizeof(RankRec)));
    HIP_CHECK(hipMalloc(&job->d_dstoff, n * sizeof(uint64_t)));
    HIP_CHECK(hipMalloc(&job->d_pos, n * sizeof(uint32_t)));
    HIP_CHECK(hipMalloc(&job->d_outindex, n * 16));
    HIP_CHECK(hipMalloc(&job->d_srcmap, n * sizeof(uint64_t)));
    HIP_CHECK(hipMalloc(&job->d_outdata, total_data ? total_data : 16));
    job->n_tiles = (uint32_t)((n + EMIT_TILE - 1) / EMIT_TILE);
    HIP_CHECK(hipMalloc(&job->d_err, JOB_ERR_WORDS * sizeof(uint32_t) +
                                         job->n_tiles * sizeof(uint64_t)));
    job->d_needwin = job->d_err + 2;
    job->d_tilesum = (uint64_t*)(job->d_err + JOB_ERR_WORDS);
    HIP_CHECK(hipMalloc(&job->d_pfx, n * sizeof(uint64_t)));
    HIP_CHECK(hipMalloc(&job->d_tot, sizeof(StepTotals)));
    HIP_CHECK(hipHostMalloc(&job->h_tot, sizeof(StepTotals)));
    uint32_t max_job_runs = 1;
    {
        for (size_t j = 0; j < n_jobs; j++)
            if (runs_per_job[j] > max_job_runs)
                max_job_runs = runs_per_job[j];
    }
    HIP_CHECK(hipMalloc(&job->d_cr,
                        (max_job_runs > 1 ? (max_job_runs - 1) * n : 1) *
                            4));
    /* sized for the smallest copy-window variant (8 KiB) */
    HIP_CHECK(hipMalloc(&job->d_winp0,
                        (total_data / 8192 + 2) * sizeof(uint32_t)));

    HIP_CHECK(survivor_scans(nullptr, job->scantmp_bytes, job->d_rank,
                             job->d_dstoff, job->d_pos, n, job->stream));
    HIP_CHECK(hipMalloc(&job->d_scantmp, job->scantmp_bytes));

    /* Upload: one slab; record per-run device pointers. */
    HIP_CHECK(hipEventRecord(job->ev[0], job->stream));
    uint8_t* p = borrowed ? nullptr : job->d_input + 16;
    RunsDesc& D = job->desc;
    memset(&D, 0, sizeof D);
    D.n_runs = (int)n_runs;
    D.total = total;
    {
        uint32_t r0 = 0;
        for (size_t j = 0; j < n_jobs; j++) {
            for (uint32_t r = r0; r < r0 + runs_per_job[j]; r++) {
                D.job_lo[r] = (uint8_t)r0;
                D.job_hi[r] = (uint8_t)(r0 + runs_per_job[j]);
            }
            r0 += runs_per_job[j];
        }
    }
    uint64_t base = 0;
    for (size_t r = 0; r < n_runs; r++) {
        D.data[r] = borrowed ? runs[r].data : p;
        D.data_len[r] = runs[r].data_len;
        if (runs[r].data_len && !borrowed) {
            HIP_CHECK(hipMemcpyAsync(p, runs[r].data, runs[r].data_len,
                                     hipMemcpyHostToDevice, job->stream));
            p += runs[r].data_len;
        }
        D.index[r] = borrowed ? runs[r].index : p;
        D.count[r] = runs[r].index_len / 16;
        if (runs[r].index_len && !borrowed) {
            HIP_CHECK(hipMemcpyAsync(p, runs[r].index, runs[r].index_len,
                                     hipMemcpyHostToDevice, job->stream));
            if (off_bias && off_bias[r])
                hipLaunchKernelGGL(k_index_rebase,
                                   dim3(pick_grid(D.count[r], 256)),
                                   dim3(256), 0, job->stream, p, D.count[r],
                                   (uint64_t)0 - off_bias[r]);
            p += runs[r].index_len;
        }
        D.entry_base[r] = base;
        base += D.count[r];
    }
    /* merge-path pair table: one entry per unordered run pair with work */
    {
        /* 32 KiB on the stack: nothing to allocate, nothing to fail */
        PairDesc hp[MAX_RUNS * (MAX_RUNS - 1) / 2];
        uint64_t cbase = 0;
        uint32_t np = 0;
        for (uint32_t a = 0; a < n_runs; a++)
            for (uint32_t b = a + 1; b < D.job_hi[a]; b++) {
                uint64_t len = D.count[a] + D.count[b];
                if (!len) continue;
                hp[np++] = {a, b, cbase};
                cbase += (len + CORANK_BLOCK_POS - 1) / CORANK_BLOCK_POS;
            }
        job->n_pairs = np;
        job->total_chunks = cbase;
        HIP_CHECK(hipMalloc(&job->d_corners, (cbase ? cbase : 1) * 8));
        if (np) {
            HIP_CHECK(hipMalloc(&job->d_pairs, np * sizeof(PairDesc)));
            HIP_CHECK(hipMemcpy(job->d_pairs, hp, np * sizeof(PairDesc),
                                hipMemcpyHostToDevice));
        }
    }
    {
        uint32_t r0 = 0;
        for (size_t j = 0; j < n_jobs; j++) {
            job->job_gbase.push_back(D.entry_base[r0]);
            r0 += runs_per_job[j];
        }
        job->job_gbase.push_back(total);
    }
    HIP_CHECK(hipEventRecord(job->ev[1], job->stream));
    HIP_CHECK(hipStreamSynchronize(job->stream));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, job->ev[0], job->ev[1]));
    job->h2d_ms = borrowed ? 0.0 : ms;

    /* pick the aux tier from the max key_size (index slabs are resident
     * now); the tier is a traffic optimization only — every tier is
     * correct for every key length (blob fallback on deep ties) */
    if (total) {
        HIP_CHECK(hipMemsetAsync(job->d_err, 0, 8, job->stream));
        hipLaunchKernelGGL(k_maxks, dim3(pick_grid(total, 256)), dim3(256),
                           0, job->stream, job->desc, job->d_err + 1);
        uint32_t maxks = 0;
        HIP_CHECK(hipMemcpyAsync(&maxks, job->d_err + 1, 4,
                                 hipMemcpyDeviceToHost, job->stream));
        HIP_CHECK(hipStreamSynchronize(job->stream));
        uint32_t maxklen = maxks > 8 ? maxks - 8 : 0;
        job->aux_kind = maxklen <= 20 ? 0 : (maxklen <= 32 ? 1 : 2);
    } else {
        job->aux_kind = 0;
    }
    uint64_t aux_sz = 0;
    with_aux_tier(job->aux_kind, [&](auto tier) {
        aux_sz = sizeof(typename decltype(tier)::Rec);
    });
    HIP_CHECK(hipMalloc(&job->d_aux, n * aux_sz));

    drop_job.dismiss();
    *out_job = job;
    return DBEEL_OK;
}

extern "C" int dbeel_gpu_job_create(const dbeel_run_view* runs,
                                    size_t n_runs, int device,
                                    dbeel_gpu_job** out_job) {
    uint32_t one[1] = {(uint32_t)n_runs};
    return job_create_impl(runs, n_runs, one, 1, device, out_job);
}

/* Batched independent jobs in ONE launch set (BASELINE configs[3]'s
 * 8-jobs-per-GPU shape): runs[] holds every job's runs back to back,
 * runs_per_job[] their counts. Jobs never pair with each other (ranks,
 * crossranks and winner flags are job-local); outputs land concatenated
 * in job order and dbeel_gpu_job_fetch_job slices them back out. One
 * kernel pipeline per step replaces 8 per-stream pipelines' launch
 * storms and partial-fill tails. */
extern "C" int dbeel_gpu_job_create_batched(const dbeel_run_view* runs,
                                            size_t n_runs,
                                            const uint32_t* runs_per_job,
                                            size_t n_jobs, int device,
                                            dbeel_gpu_job** out_job) {
    if (!runs_per_job || !n_jobs) {
        set_err("runs_per_job is null/empty");
        return DBEEL_ERR_INVALID_ARG;
    }
    return job_create_impl(runs, n_runs, runs_per_job, n_jobs, device,
                           out_job);
}

/* Per-job slice of a batched job's last result: data/index of job
 * `job_idx`, index offsets rebased to the job's own run file. */
extern "C" int dbeel_gpu_job_fetch_job(dbeel_gpu_job* job, size_t job_idx,
                                       dbeel_compact_result* out) {
    g_err[0] = 0;
    if (!job || !out || !job->have_result ||
        job_idx + 1 >= job->job_gbase.size()) {
        set_err("fetch_job: no result / bad job index");
        return DBEEL_ERR_INVALID_ARG;
    }
    HIP_CHECK(hipSetDevice(job->device));
    memset(out, 0, sizeof *out);
    uint64_t g0 = job->job_gbase[job_idx];
    uint64_t g1 = job->job_gbase[job_idx + 1];
    /* boundary offsets/positions: tiny D2H reads (packed scan mode
     * carries both in one u64 — decode below) */
    uint64_t off0 = 0, off1 = job->out_data_len;
    uint32_t pos0 = 0, pos1 = (uint32_t)job->out_entries;
    hipStream_t s = job->stream;
    int pk = job->last_scan_packed;
    if (pk == 2) {
        /* tile mode kept no per-entry values: rebuild the two asked for,
         * into the slots the rocPRIM scan would have left them in */
        if (g0 > 0)
            hipLaunchKernelGGL(k_tile_value_at, dim3(1), dim3(EMIT_BLOCK),
                               0, s, job->d_rank, job->d_tilesum, g0,
                               job->d_dstoff + g0);
        if (g1 < job->total_entries)
            hipLaunchKernelGGL(k_tile_value_at, dim3(1), dim3(EMIT_BLOCK),
                               0, s, job->d_rank, job->d_tilesum, g1,
                               job->d_dstoff + g1);
    }
    if (g0 > 0) {
        HIP_CHECK(hipMemcpyAsync(&off0, job->d_dstoff + g0, 8,
                                 hipMemcpyDeviceToHost, s));
        if (!pk)
            HIP_CHECK(hipMemcpyAsync(&pos0, job->d_pos + g0, 4,
                                     hipMemcpyDeviceToHost, s));
    }
    if (g1 < job->total_entries) {
        HIP_CHECK(hipMemcpyAsync(&off1, job->d_dstoff + g1, 8,
                                 hipMemcpyDeviceToHost, s));
        if (!pk)
            HIP_CHECK(hipMemcpyAsync(&pos1, job->d_pos + g1, 4,
                                     hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
    if (pk) {
        if (g0 > 0) {
            pos0 = (uint32_t)(off0 >> PK_SHIFT);
            off0 &= PK_MASK;
        }
        if (g1 < job->total_entries) {
            pos1 = (uint32_t)(off1 >> PK_SHIFT);
            off1 &= PK_MASK;
        }
    }
    uint64_t dlen = off1 - off0;
    uint64_t nsurv = (uint64_t)pos1 - pos0;
    out->data = (uint8_t*)malloc(dlen ? dlen : 1);
    out->index = (uint8_t*)malloc(nsurv ? nsurv * 16 : 1);
    if (!out->data || !out->index) {
        free(out->data);
        free(out->index);
        memset(out, 0, sizeof *out);
        set_err("host malloc failed");
        return DBEEL_ERR_OOM;
    }
    hipError_t ce = hipSuccess;
    if (dlen)
        ce = hipMemcpyAsync(out->data, job->d_outdata + off0, dlen,
                            hipMemcpyDeviceToHost, s);
    if (ce == hipSuccess && nsurv)
        ce = hipMemcpyAsync(out->index,
                            job->d_outindex + (uint64_t)pos0 * 16,
                            nsurv * 16, hipMemcpyDeviceToHost, s);
    if (ce == hipSuccess) ce = hipStreamSynchronize(s);
    if (ce != hipSuccess) {
        free(out->data);
        free(out->index);
        memset(out, 0, sizeof *out);
        set_err("fetch_job D2H failed: %s", hipGetErrorString(ce));
        return DBEEL_ERR_HIP;
    }
    /* rebase offsets to the job's own file */
    for (uint64_t i = 0; i < nsurv; i++) {
        uint64_t o = ld_u64_host(out->index + i * 16) - off0;
        memcpy(out->index + i * 16, &o, 8);
    }
    out->data_len = dlen;
    out->index_len = nsurv * 16;
    out->entries_written = nsurv;
    return DBEEL_OK;
}

extern "C" void dbeel_gpu_job_destroy(dbeel_gpu_job* job) {
    if (!job) return;
    if (job->device >= 0) hipSetDevice(job->device);
    hipFree(job->d_input); /* null for a borrowed-input job */
    hipFree(job->d_rank);
    hipFree(job->d_dstoff);
    hipFree(job->d_pos);
    hipFree(job->d_outindex);
    hipFree(job->d_srcmap);
    hipFree(job->d_outdata);
    hipFree(job->d_scantmp);
    hipFree(job->d_err);
    hipFree(job->d_pfx);
    hipFree(job->d_aux);
    hipFree(job->d_cr);
    hipFree(job->d_pairs);
    hipFree(job->d_winp0);
    hipFree(job->d_corners);
    hipFree(job->d_tot);
    if (job->h_tot) hipHostFree(job->h_tot);
    for (int i = 0; i < 8; i++)
        if (job->ev[i]) hipEventDestroy(job->ev[i]);
    if (job->stream) hipStreamDestroy(job->stream);
    if (job->copy_stream) hipStreamDestroy(job->copy_stream);
    delete job;
}

/* ------------------------------------------------------------------ */
/* Streamed pinned ingest (north_star: pinned host DRAM, chunked       */
/* hipMemcpyAsync, compute overlap). See include/dbeel_gpu.h.          */
/* ------------------------------------------------------------------ */

extern "C" int dbeel_gpu_pin_host(const void* ptr, size_t len) {
    g_err[0] = 0;
    if (!ptr || !len) {
        set_err("pin_host: null/empty buffer");
        return DBEEL_ERR_INVALID_ARG;
    }
    hipError_t e = hipHostRegister(const_cast<void*>(ptr), len,
                                   hipHostRegisterDefault);
    if (e == hipErrorHostMemoryAlreadyRegistered) return DBEEL_OK;
    if (e != hipSuccess) {
        set_err("hipHostRegister failed: %s", hipGetErrorString(e));
        return DBEEL_ERR_HIP;
    }
    return DBEEL_OK;
}

extern "C" int dbeel_gpu_unpin_host(const void* ptr) {
    g_err[0] = 0;
    hipError_t e = hipHostUnregister(const_cast<void*>(ptr));
    if (e != hipSuccess && e != hipErrorHostMemoryNotRegistered) {
        set_err("hipHostUnregister failed: %s", hipGetErrorString(e));
        return DBEEL_ERR_HIP;
    }
    return DBEEL_OK;
}

/* k_prepare over the global entries [g0, g1) in the job's aux tier. */
static void launch_prepare(dbeel_gpu_job* job, uint64_t g0, uint64_t g1,
                           hipStream_t s) {
    with_aux_tier(job->aux_kind, [&](auto tier) {
        using T = decltype(tier);
        hipLaunchKernelGGL((k_prepare<T::KB, T::TS>),
                           dim3(pick_grid(g1 - g0, 256)), dim3(256), 0, s,
                           job->desc, g0, g1, job->d_pfx,
                           (typename T::Rec*)job->d_aux, job->d_err);
    });
}

extern "C" int dbeel_gpu_job_ingest(dbeel_gpu_job* job,
                                    const dbeel_run_view* runs,
                                    size_t n_runs,
                                    dbeel_ingest_stats* stats) {
    g_err[0] = 0;
    if (!job || !runs) {
        set_err("job_ingest: null argument");
        return DBEEL_ERR_INVALID_ARG;
    }
    if (job->borrowed) {
        set_err("job_ingest: the job's inputs belong to a resident reader");
        return DBEEL_ERR_INVALID_ARG;
    }
    if ((int)n_runs != job->desc.n_runs) {
        set_err("job_ingest: run count %zu != job's %d", n_runs,
                job->desc.n_runs);
        return DBEEL_ERR_INVALID_ARG;
    }
    int rc = validate_runs(runs, n_runs);
    if (rc) return rc;
    for (size_t r = 0; r < n_runs; r++) {
        if (runs[r].data_len != job->desc.data_len[r] ||
            runs[r].index_len / 16 != job->desc.count[r]) {
            set_err("job_ingest: run %zu shape differs from the job's", r);
            return DBEEL_ERR_INVALID_ARG;
        }
    }
    HIP_CHECK(hipSetDevice(job->device));
    if (!job->copy_stream) HIP_CHECK(hipStreamCreate(&job->copy_stream));
    hipStream_t cs = job->copy_stream; /* H2D lane */
    hipStream_t ks = job->stream;      /* compute lane */
    job->prep_valid = 0;
    job->have_result = false;

    uint64_t chunk_bytes = 64ull << 20;
    if (const char* c = getenv("DBEEL_STREAM_CHUNK_MB")) {
        long v = atol(c);
        if (v >= 1) chunk_bytes = (uint64_t)v << 20;
    }

    /* chunk events: copies are in-order on cs, so event i implies all
     * earlier chunks arrived */
    std::vector<hipEvent_t> evs;
    hipEvent_t ev_cs0 = nullptr, ev_cs1 = nullptr, ev_ks0 = nullptr,
               ev_ks1 = nullptr;
    ScopeGuard destroy_events([&] {
        for (hipEvent_t e : evs) hipEventDestroy(e);
        for (hipEvent_t e : {ev_cs0, ev_cs1, ev_ks0, ev_ks1})
            if (e) hipEventDestroy(e);
    });
    HIP_CHECK(hipEventCreate(&ev_cs0));
    HIP_CHECK(hipEventCreate(&ev_cs1));
    HIP_CHECK(hipEventCreate(&ev_ks0));
    HIP_CHECK(hipEventCreate(&ev_ks1));
    HIP_CHECK(hipMemsetAsync(job->d_err, 0, 8, ks));

    HIP_CHECK(hipEventRecord(ev_cs0, cs));
    HIP_CHECK(hipEventRecord(ev_ks0, ks));
    uint64_t total_chunks = 0;

    /* index slabs first (small; prepare reads them for every entry) */
    for (size_t r = 0; r < n_runs; r++) {
        if (!runs[r].index_len) continue;
        HIP_CHECK(hipMemcpyAsync(
            const_cast<uint8_t*>(job->desc.index[r]), runs[r].index,
            runs[r].index_len, hipMemcpyHostToDevice, cs));
    }
    {
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        evs.push_back(e);
        HIP_CHECK(hipEventRecord(e, cs));
        HIP_CHECK(hipStreamWaitEvent(ks, e, 0));
    }

    /* stream each run's data in entry-aligned chunks; launch the ranged
     * prepare for a chunk's entries as soon as its bytes are on device */
    for (size_t r = 0; r < n_runs; r++) {
        uint64_t n = job->desc.count[r];
        uint64_t dlen = runs[r].data_len;
        if (!dlen) {
            /* entries with no data bytes are corrupt; the ranged prepare
             * must still run over them so the corruption is FLAGGED (it
             * is normally launched per data chunk) */
            if (n) {
                uint64_t g0 = job->desc.entry_base[r];
                launch_prepare(job, g0, g0 + n, ks);
            }
            continue;
        }
        const uint8_t* hidx = runs[r].index;
        uint64_t e0 = 0, b0 = 0;
        while (b0 < dlen) {
            uint64_t btarget = b0 + chunk_bytes;
            uint64_t e1, b1;
            if (btarget >= dlen) {
                e1 = n;
                b1 = dlen;
            } else {
                /* first entry with offset >= btarget (offsets monotone,
                 * non-overlapping — verified on-device by k_prepare) */
                uint64_t lo = e0, hi = n;
                while (lo < hi) {
                    uint64_t mid = (lo + hi) >> 1;
                    if (ld_u64_host(hidx + mid * 16) < btarget)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                e1 = lo;
                b1 = (e1 >= n) ? dlen : ld_u64_host(hidx + e1 * 16);
                if (e1 >= n) e1 = n;
                if (b1 <= b0) { /* one giant entry spans the chunk */
                    e1 = e0 + 1;
                    b1 = (e1 >= n) ? dlen : ld_u64_host(hidx + e1 * 16);
                }
                /* corrupt (non-monotone) offsets could still point
                 * backwards or past the run: clamp to a safe single
                 * tail chunk — the on-device validation then reports
                 * CORRUPT instead of this loop wrapping a copy size */
                if (b1 <= b0 || b1 > dlen) {
                    e1 = n;
                    b1 = dlen;
                }
            }
            HIP_CHECK(hipMemcpyAsync(
                const_cast<uint8_t*>(job->desc.data[r]) + b0,
                runs[r].data + b0, b1 - b0, hipMemcpyHostToDevice, cs));
            hipEvent_t e;
            HIP_CHECK(hipEventCreate(&e));
            evs.push_back(e);
            HIP_CHECK(hipEventRecord(e, cs));
            HIP_CHECK(hipStreamWaitEvent(ks, e, 0));
            if (e1 > e0)
                launch_prepare(job, job->desc.entry_base[r] + e0,
                               job->desc.entry_base[r] + e1, ks);
            total_chunks++;
            e0 = e1;
            b0 = b1;
        }
    }

    HIP_CHECK(hipEventRecord(ev_cs1, cs));
    HIP_CHECK(hipEventRecord(ev_ks1, ks));
    uint32_t err = 0;
    HIP_CHECK(hipMemcpyAsync(&err, job->d_err, 4, hipMemcpyDeviceToHost,
                             ks));
    HIP_CHECK(hipStreamSynchronize(cs));
    HIP_CHECK(hipStreamSynchronize(ks));
    HIP_CHECK(hipGetLastError());
    if (err) {
        set_err("corrupt entry/index record in streamed ingest");
        return DBEEL_ERR_CORRUPT;
    }

    if (stats) {
        float copy_ms = 0, prep_ms = 0, wall_ms = 0;
        (void)hipEventElapsedTime(&copy_ms, ev_cs0, ev_cs1);
        (void)hipEventElapsedTime(&prep_ms, ev_ks0, ev_ks1);
        (void)hipEventElapsedTime(&wall_ms, ev_cs0, ev_ks1);
        if (prep_ms > wall_ms) wall_ms = prep_ms;
        stats->ingest_ms = wall_ms;
        stats->copy_ms = copy_ms;
        stats->prep_ms = prep_ms;
        stats->bytes = job->input_bytes;
        stats->chunks = total_chunks;
    }
    job->h2d_ms = 0.0; /* transfer accounted in ingest stats */
    job->prep_valid = 1;
    return DBEEL_OK;
}

extern "C" uint32_t dbeel_gpu_grid_for(uint64_t work_items, uint32_t block) {
    return block ? pick_grid(work_items, block) : 0;
}

/* Copy-geometry selection measured by interleaved A/B (tools/ab_copy.py,
 * r02): ~1 KiB survivors (cfg3) run 11% faster with 64 KiB windows /
 * 512 threads (fewer window transitions+barriers per block); 4 KiB
 * survivors (cfg5) want MORE blocks (grid 16384) at the default window
 * (the 4096 cap left most waves parked); sub-512-B survivors keep the
 * default. Env DBEEL_COPY_VARIANT / DBEEL_COPY_GRID override for A/Bs.
 *
 * The real totals live on the device (StepTotals), so the host decides
 * from what it knows before the step: the grid from an upper bound on the
 * output (the input's data bytes; surplus blocks and windows exit), the
 * variant from the INPUT's average entry size. The three classes are wide
 * (< 512, 512..2048, > 2048 B) and the BASELINE shapes sit well inside
 * them on both measures (cfg2/cfg4 304 B in, 304 B out; cfg3 1037 B in,
 * 1088 B out; cfg5 ~4.07 KiB in, ~4.15 KiB out), so this picks what the
 * output average picked. The two can differ only when dropped tombstones
 * or superseded entries shift the average across a class boundary (say
 * 60% dropped tombstones among 1 KiB values: 470 B in, 1088 B out); every
 * variant is correct for every size, the choice is a speed matter only. */
struct CopyGeom {
    int variant;
    uint32_t win, blk;
    uint64_t gcap;
    uint64_t windows; /* upper bound, from the input bytes */
};

static CopyGeom copy_geometry(uint64_t in_entries, uint64_t in_bytes) {
    int variant = -1;
    if (const char* v = getenv("DBEEL_COPY_VARIANT")) variant = atoi(v);
    uint64_t gcap = 0;
    if (const char* g = getenv("DBEEL_COPY_GRID")) {
        long v = atol(g);
        if (v >= 64) gcap = (uint64_t)v;
    }
    if (variant < 0) {
        uint64_t avg = in_entries ? in_bytes / in_entries : 0;
        if (avg > 2048) {
            variant = 0; /* 4 KiB-class: more blocks, small windows */
            if (!gcap) gcap = 16384;
        } else if (avg >= 512) {
            variant = 4; /* ~1 KiB-class: 64 KiB windows */
        } else {
            variant = 3; /* sub-512-B: 512thr x 32 KiB + more blocks
                            (cfg2 A/B: 0.516 -> 0.467 ms) */
            if (!gcap) gcap = 16384;
        }
    }
    if (!gcap) gcap = 4096;
    uint32_t win = (variant == 1)   ? 8192
                   : (variant == 3) ? 32768
                   : (variant == 4) ? 65536
                                    : 16384;
    uint32_t blk = (variant >= 2) ? 512 : 256;
    /* every window size is a power of two: k_emit_tile shifts by it */
    return CopyGeom{variant, win, blk, gcap, (in_bytes + win - 1) / win};
}

/* need_winmap: null, or a device flag that is clear when the emit kernel
 * has filled win_p0 itself (k_emit_tile); k_winmap then returns at once. */
static void launch_copy(hipStream_t s, const uint8_t* out_index,
                        const uint64_t* src_map, uint32_t* win_p0,
                        const StepTotals* tot, uint64_t in_entries,
                        uint64_t in_bytes, uint8_t* out_data,
                        const uint32_t* need_winmap = nullptr) {
    const CopyGeom G = copy_geometry(in_entries, in_bytes);
    const int variant = G.variant;
    const uint32_t win = G.win, blk = G.blk;
    const uint64_t windows = G.windows, gcap = G.gcap;
    if (!windows) return;
    uint32_t grid = windows > gcap ? (uint32_t)gcap : (uint32_t)windows;
    hipLaunchKernelGGL(k_winmap, dim3(pick_grid(windows, 256)), dim3(256),
                       0, s, out_index, tot, win, win_p0, need_winmap);
    void (*kc)(const uint8_t*, const uint64_t*, const uint32_t*,
               const StepTotals*, uint8_t*) = k_copy<256, 16384>;
    if (variant == 1) kc = k_copy<256, 8192>;
    if (variant == 2) kc = k_copy<512, 16384>;
    if (variant == 3) kc = k_copy<512, 32768>;
    if (variant == 4) kc = k_copy<512, 65536>;
    hipLaunchKernelGGL(kc, dim3(grid), dim3(blk), 0, s, out_index, src_map,
                       win_p0, tot, out_data);
}

extern "C" int dbeel_gpu_job_run(dbeel_gpu_job* job, int keep_tombstones,
                                 uint64_t* out_data_len,
                                 uint64_t* out_entries,
                                 dbeel_compact_timings* t) {
    g_err[0] = 0;
    if (!job) {
        set_err("job is null");
        return DBEEL_ERR_INVALID_ARG;
    }
    HIP_CHECK(hipSetDevice(job->device));
    hipStream_t s = job->stream;
    uint64_t n = job->total_entries;
    job->have_result = false;

    int skip_prep = job->prep_valid;
    /* How the survivor offsets are made. Packed (one u64 carries bytes and
     * count) where the job fits its bounds; there by rank tile unless
     * DBEEL_SCAN_MODE=rocprim asks for the per-entry rocPRIM scan, for
     * A/B. DBEEL_SCAN_MODE=two forces the two-scan form of larger jobs. */
    bool packed = n < (1ull << 26) &&
                  job->total_data_bytes < (1ull << PK_SHIFT);
    bool tiled = packed;
    if (const char* m = getenv("DBEEL_SCAN_MODE")) {
        if (!strcmp(m, "two")) packed = tiled = false;
        if (!strcmp(m, "rocprim")) tiled = false;
    }
    HIP_CHECK(hipMemsetAsync(
        job->d_err, 0,
        tiled ? JOB_ERR_WORDS * sizeof(uint32_t) +
                    job->n_tiles * sizeof(uint64_t)
              : 2 * sizeof(uint32_t),
        s));

    HIP_CHECK(hipEventRecord(job->ev[0], s));
    if (n && !skip_prep) launch_prepare(job, 0, n, s);
    HIP_CHECK(hipEventRecord(job->ev[6], s));
    if (n) {
        uint32_t grid = pick_grid(n, 256);
        uint64_t cgrid = job->total_chunks;
        if (cgrid > 16384) cgrid = 16384;
        if (const char* g = getenv("DBEEL_CORANK_GRID")) {
            long v = atol(g); /* fewer blocks: several windows per block */
            if (v >= 1 && (uint64_t)v < cgrid) cgrid = (uint64_t)v;
        }
        int corank_wide = 0; /* A/B: 512-thread corank blocks */
        if (const char* w = getenv("DBEEL_CORANK_BLOCK"))
            corank_wide = atoi(w) >= 512;
        with_aux_tier(job->aux_kind, [&](auto tier) {
            using T = decltype(tier);
            constexpr int KB = T::KB;
            constexpr bool TS = T::TS;
            const typename T::Rec* aux = (const typename T::Rec*)job->d_aux;
            const PairDesc* pairs = (const PairDesc*)job->d_pairs;
            if (job->n_pairs) {
                hipLaunchKernelGGL((k_corners<KB, TS>),
                                   dim3(pick_grid(job->total_chunks, 256)),
                                   dim3(256), 0, s, job->desc, job->d_pfx,
                                   aux, pairs, job->n_pairs,
                                   job->total_chunks, job->d_corners);
                if (corank_wide)
                    hipLaunchKernelGGL((k_corank<KB, TS, 512>),
                                       dim3((uint32_t)cgrid), dim3(512), 0, s,
                                       job->desc, job->d_pfx, aux, pairs,
                                       job->n_pairs, job->total_chunks,
                                       job->d_corners, job->d_cr);
                else
                    hipLaunchKernelGGL((k_corank<KB, TS, 256>),
                                       dim3((uint32_t)cgrid),
                                       dim3(CORANK_BLOCK), 0, s, job->desc,
                                       job->d_pfx, aux, pairs, job->n_pairs,
                                       job->total_chunks, job->d_corners,
                                       job->d_cr);
            }
            hipLaunchKernelGGL((k_rankreduce<KB, TS>), dim3(grid), dim3(256),
                               0, s, job->desc, job->d_pfx, aux, job->d_cr,
                               job->d_rank, keep_tombstones, job->d_err,
                               tiled ? job->d_tilesum : nullptr);
        });
    }
    HIP_CHECK(hipEventRecord(job->ev[1], s));
    const CopyGeom geom = copy_geometry(n, job->total_data_bytes);
    if (n) {
        size_t tmp = job->scantmp_bytes;
        if (tiled)
            hipLaunchKernelGGL(k_tilebase, dim3(1), dim3(TILEBASE_BLOCK), 0,
                               s, job->d_tilesum, job->n_tiles);
        else if (packed)
            HIP_CHECK(rocprim::exclusive_scan(
                job->d_scantmp, tmp,
                rocprim::make_transform_iterator(job->d_rank,
                                                 RankRecPacked{}),
                job->d_dstoff, (uint64_t)0, n, rocprim::plus<uint64_t>(),
                s));
        else
            HIP_CHECK(survivor_scans(job->d_scantmp, tmp, job->d_rank,
                                     job->d_dstoff, job->d_pos, n, s));
    }
    HIP_CHECK(hipEventRecord(job->ev[2], s));
    if (n) {
        uint32_t grid = pick_grid(n, 256);
        if (tiled)
            hipLaunchKernelGGL(k_emit_tile, dim3(job->n_tiles),
                               dim3(EMIT_BLOCK), 0, s, job->desc,
                               job->d_rank, job->d_tilesum, n,
                               job->d_outindex, job->d_srcmap, job->d_err,
                               job->d_tot,
                               (uint32_t)__builtin_ctz(geom.win),
                               geom.windows, job->d_winp0, job->d_needwin);
        else if (packed)
            hipLaunchKernelGGL(k_emit_packed, dim3(grid), dim3(256), 0, s,
                               job->desc, job->d_rank, job->d_dstoff, n,
                               job->d_outindex, job->d_srcmap, job->d_err,
                               job->d_tot);
        else
            hipLaunchKernelGGL(k_emit, dim3(grid), dim3(256), 0, s,
                               job->desc, job->d_rank, job->d_dstoff,
                               job->d_pos, n, job->d_outindex,
                               job->d_srcmap, job->d_err, job->d_tot);
    } else {
        HIP_CHECK(hipMemsetAsync(job->d_tot, 0, sizeof(StepTotals), s));
    }
    HIP_CHECK(hipEventRecord(job->ev[3], s));

    /* The copy takes its totals from the device record: nothing to wait
     * for here. One sync and one 24-B read end the step. */
    HIP_CHECK(hipEventRecord(job->ev[4], s));
    if (n)
        launch_copy(s, job->d_outindex, job->d_srcmap, job->d_winp0,
                    job->d_tot, n, job->total_data_bytes, job->d_outdata,
                    tiled ? job->d_needwin : nullptr);
    HIP_CHECK(hipEventRecord(job->ev[5], s));
    HIP_CHECK(hipMemcpyAsync(job->h_tot, job->d_tot, sizeof(StepTotals),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    uint32_t err = (uint32_t)job->h_tot->err;
    if (err) {
        set_err(err & DERR_UNSORTED
                    ? "input run not strictly sorted by unique keys "
                      "(dbeel flush invariant violated)"
                    : "corrupt entry/index record");
        return DBEEL_ERR_CORRUPT;
    }
    job->last_scan_packed = tiled ? 2 : packed ? 1 : 0;
    uint64_t total_out = job->h_tot->total_out;
    uint64_t n_surv = job->h_tot->n_surv;

    job->out_data_len = total_out;
    job->out_entries = n_surv;
    job->have_result = true;
    if (out_data_len) *out_data_len = total_out;
    if (out_entries) *out_entries = n_surv;
    if (t) {
        float prep_ms = 0, rank_ms = 0, scan_ms = 0, emit_ms = 0,
              copy_ms = 0;
        (void)hipEventElapsedTime(&prep_ms, job->ev[0], job->ev[6]);
        (void)hipEventElapsedTime(&rank_ms, job->ev[6], job->ev[1]);
        (void)hipEventElapsedTime(&scan_ms, job->ev[1], job->ev[2]);
        (void)hipEventElapsedTime(&emit_ms, job->ev[2], job->ev[3]);
        (void)hipEventElapsedTime(&copy_ms, job->ev[4], job->ev[5]);
        t->h2d_ms = job->h2d_ms;
        t->prep_ms = prep_ms;
        t->rank_ms = rank_ms;
        t->scan_ms = scan_ms;
        t->emit_ms = emit_ms;
        t->copy_ms = copy_ms;
        t->kernel_ms = prep_ms + rank_ms + scan_ms + emit_ms + copy_ms;
        t->d2h_ms = 0.0;
    }
    return DBEEL_OK;
}

/* ------------------------------------------------------------------ */
/* Bloom builder (behavioral filter over the surviving keys)          */
/*                                                                    */
/* The reference builds a bloomfilter::Bloom over every written key   */
/* (lsm_tree.rs:1026-1051); its file bytes are unpinnable (random     */
/* SipHash keys), so this engine ships its own "DBLM" format — same   */
/* behavior (zero false negatives, ~1% fp at k=7), built here on the  */
/* device from the job's resident output. Hash = seeded FNV-1a 64     */
/* with a splitmix64 finalizer, identical to dbeel_lsm.cpp's checker. */
/* ------------------------------------------------------------------ */

/* The filter parameters every device-built "DBLM" shares: sized for 1% fp
 * (BLOOM_MAX_ALLOWED_ERROR, lsm_tree.rs:48) at k = 7. */
#define BLOOM_K 7u
#define BLOOM_SEED 0xDBEE1ull
static inline uint64_t bloom_bits_for(uint64_t n_keys) {
    return (uint64_t)(9.585 * (double)(n_keys ? n_keys : 1)) + 64;
}

/* splitmix64 finalizer */
__device__ __forceinline__ uint64_t d_mix64(uint64_t h) {
    h ^= h >> 30;
    h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 27;
    h *= 0x94d049bb133111ebull;
    h ^= h >> 31;
    return h;
}

__device__ __forceinline__ uint64_t d_fnv1a64(const uint8_t* p, uint64_t n,
                                              uint64_t seed) {
    uint64_t h = 1469598103934665603ull ^ seed;
    for (uint64_t i = 0; i < n; i++) {
        h ^= p[i];
        h *= 1099511628211ull;
    }
    return d_mix64(h);
}

__global__ void k_bloom(const uint8_t* out_data, const uint8_t* out_index,
                        uint64_t n_surv, uint64_t n_bits, uint64_t seed,
                        uint32_t kk, uint32_t* bits) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n_surv; i += stride) {
        const uint8_t* rec = out_index + i * 16;
        uint64_t off = ld_u64(rec);
        uint32_t key_size = ld_u32(rec + 8);
        const uint8_t* key = out_data + off + 8;
        uint64_t klen = key_size - 8;
        uint64_t h1 = d_fnv1a64(key, klen, seed);
        uint64_t h2 =
            d_fnv1a64(key, klen, seed ^ 0x9e3779b97f4a7c15ull) | 1;
        for (uint32_t j = 0; j < kk; j++) {
            uint64_t bit = (h1 + j * h2) % n_bits;
            atomicOr(&bits[bit >> 5], 1u << (bit & 31));
        }
    }
}

extern "C" int dbeel_gpu_job_bloom(dbeel_gpu_job* job, uint8_t** out_bytes,
                                   uint64_t* out_len) {
    g_err[0] = 0;
    if (!job || !out_bytes || !out_len || !job->have_result) {
        set_err("job_bloom: no result available");
        return DBEEL_ERR_INVALID_ARG;
    }
    HIP_CHECK(hipSetDevice(job->device));
    uint64_t n_bits = bloom_bits_for(job->out_entries);
    uint64_t n_words = (n_bits + 31) / 32;
    uint32_t* d_bits = nullptr;
    HIP_CHECK(hipMalloc(&d_bits, n_words * 4));
    HIP_CHECK(hipMemsetAsync(d_bits, 0, n_words * 4, job->stream));
    if (job->out_entries)
        hipLaunchKernelGGL(k_bloom, dim3(pick_grid(job->out_entries, 256)),
                           dim3(256), 0, job->stream, job->d_outdata,
                           job->d_outindex, job->out_entries, n_bits,
                           (uint64_t)BLOOM_SEED, BLOOM_K, d_bits);
    /* "DBLM" | ver | k | pad | n_bits | seed | bitmap (dbeel_lsm.h) */
    uint64_t blen = 32 + ((n_bits + 7) / 8);
    uint8_t* buf = (uint8_t*)calloc(1, blen + 4);
    if (!buf) {
        hipFree(d_bits);
        set_err("host alloc failed");
        return DBEEL_ERR_OOM;
    }
    memcpy(buf, "DBLM", 4);
    uint32_t ver = 1, kk = BLOOM_K, pad = 0;
    memcpy(buf + 4, &ver, 4);
    memcpy(buf + 8, &kk, 4);
    memcpy(buf + 12, &pad, 4);
    memcpy(buf + 16, &n_bits, 8);
    uint64_t seed = BLOOM_SEED;
    memcpy(buf + 24, &seed, 8);
    hipError_t e = hipMemcpyAsync(buf + 32, d_bits, (n_bits + 7) / 8,
                                  hipMemcpyDeviceToHost, job->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(job->stream);
    hipFree(d_bits);
    if (e != hipSuccess) {
        free(buf);
        set_err("bloom D2H failed: %s", hipGetErrorString(e));
        return DBEEL_ERR_HIP;
    }
    *out_bytes = buf;
    *out_len = blen;
    return DBEEL_OK;
}

extern "C" void dbeel_gpu_bloom_free(uint8_t* p) { free(p); }

extern "C" int dbeel_gpu_job_fetch(dbeel_gpu_job* job,
                                   dbeel_compact_result* out) {
    g_err[0] = 0;
    if (!job || !out || !job->have_result) {
        set_err("job_fetch: no result available");
        return DBEEL_ERR_INVALID_ARG;
    }
    HIP_CHECK(hipSetDevice(job->device));
    memset(out, 0, sizeof *out);
    uint64_t dlen = job->out_data_len, ilen = job->out_entries * 16;
    out->data = (uint8_t*)malloc(dlen ? dlen : 1);
    out->index = (uint8_t*)malloc(ilen ? ilen : 1);
    if (!out->data || !out->index) {
        free(out->data);
        free(out->index);
        memset(out, 0, sizeof *out);
        set_err("host malloc failed");
        return DBEEL_ERR_OOM;
    }
    if (dlen)
        HIP_CHECK(hipMemcpyAsync(out->data, job->d_outdata, dlen,
                                 hipMemcpyDeviceToHost, job->stream));
    if (ilen)
        HIP_CHECK(hipMemcpyAsync(out->index, job->d_outindex, ilen,
                                 hipMemcpyDeviceToHost, job->stream));
    HIP_CHECK(hipStreamSynchronize(job->stream));
    out->data_len = dlen;
    out->index_len = ilen;
    out->entries_written = job->out_entries;
    return DBEEL_OK;
}

/* Enqueues the copies of job's last result into data / index on the job's
 * stream, between e0 and e1, and returns without waiting. The caps have
 * been checked by the caller. With index_base != 0 the index records go
 * through d_rank — dead between runs, 16 B per input entry, so never
 * smaller than the output index — and are rebased there: d_outindex stays
 * as job_run left it. */
static int job_fetch_into_async(dbeel_gpu_job* job, uint8_t* data,
                                uint8_t* index, uint64_t index_base,
                                hipEvent_t e0, hipEvent_t e1) {
    hipStream_t s = job->stream;
    const uint64_t dlen = job->out_data_len, n = job->out_entries;
    HIP_CHECK(hipEventRecord(e0, s));
    const uint8_t* isrc = job->d_outindex;
    if (n && index_base) {
        uint8_t* scratch = (uint8_t*)job->d_rank;
        HIP_CHECK(hipMemcpyAsync(scratch, job->d_outindex, n * 16,
                                 hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_index_rebase, dim3(pick_grid(n, 256)), dim3(256),
                           0, s, scratch, n, index_base);
        isrc = scratch;
    }
    if (dlen)
        HIP_CHECK(hipMemcpyAsync(data, job->d_outdata, dlen,
                                 hipMemcpyDeviceToHost, s));
    if (n)
        HIP_CHECK(hipMemcpyAsync(index, isrc, n * 16, hipMemcpyDeviceToHost,
                                 s));
    HIP_CHECK(hipEventRecord(e1, s));
    return DBEEL_OK;
}

extern "C" int dbeel_gpu_job_fetch_into(
    dbeel_gpu_job* job, uint8_t* data, uint64_t data_cap, uint8_t* index,
    uint64_t index_cap, uint64_t index_base, uint64_t* data_len,
    uint64_t* index_len, double* d2h_ms) {
    g_err[0] = 0;
    if (data_len) *data_len = 0;
    if (index_len) *index_len = 0;
    if (d2h_ms) *d2h_ms = 0;
    if (!job || !data || !index || !data_len || !index_len) {
        set_err("job_fetch_into: null argument");
        return DBEEL_ERR_INVALID_ARG;
    }
    if (!job->have_result) {
        set_err("job_fetch_into: no result available");
        return DBEEL_ERR_INVALID_ARG;
    }
    const uint64_t dl = job->out_data_len, il = job->out_entries * 16;
    *data_len = dl;
    *index_len = il;
    if (dl > data_cap || il > index_cap) {
        set_err("job_fetch_into: output needs %llu data and %llu index "
                "bytes, caps are %llu and %llu", (unsigned long long)dl,
                (unsigned long long)il, (unsigned long long)data_cap,
                (unsigned long long)index_cap);
        return DBEEL_ERR_ITEM_TOO_LARGE;
    }
    hipStream_t s = job->stream;
    ScopeGuard fail([&] { (void)hipStreamSynchronize(s); });
    HIP_CHECK(hipSetDevice(job->device));
    int rc = job_fetch_into_async(job, data, index, index_base, job->ev[0],
                                  job->ev[1]);
    if (rc) return rc;
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, job->ev[0], job->ev[1]));
    if (d2h_ms) *d2h_ms = ms;
    fail.dismiss();
    return DBEEL_OK;
}

/* The filter across slices: k_bloom_hash appends k_bloom's two hashes of
 * every survivor of one job to hashes[2 * i], hashes[2 * i + 1]; k_bloom_fill
 * sets k_bloom's bits from them once n_bits is known. */
__global__ void k_bloom_hash(const uint8_t* out_data,
                             const uint8_t* out_index, uint64_t n_surv,
                             uint64_t seed, ulonglong2* hashes) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n_surv; i += stride) {
        const uint8_t* rec = out_index + i * 16;
        uint64_t off = ld_u64(rec);
        uint32_t key_size = ld_u32(rec + 8);
        const uint8_t* key = out_data + off + 8;
        uint64_t klen = key_size - 8;
        ulonglong2 h;
        h.x = d_fnv1a64(key, klen, seed);
        h.y = d_fnv1a64(key, klen, seed ^ 0x9e3779b97f4a7c15ull) | 1;
        hashes[i] = h;
    }
}

__global__ void k_bloom_fill(const ulonglong2* hashes, uint64_t n,
                             uint64_t n_bits, uint32_t kk, uint32_t* bits) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        ulonglong2 h = hashes[i];
        for (uint32_t j = 0; j < kk; j++) {
            uint64_t bit = (h.x + j * h.y) % n_bits;
            atomicOr(&bits[bit >> 5], 1u << (bit & 31));
        }
    }
}

/* ------------------------------------------------------------------ */
/* Batched point lookup                                               */
/*                                                                    */
/* GPU analogue of LSMTree::get over the sstables                     */
/* (lsm_tree.rs:605-723, binary search per run lsm_tree.rs:674-723):  */
/* one thread per query key binary-searches the runs newest-INDEX-    */
/* first and returns the first key match, exactly like the reference  */
/* read path (`sstables.iter().rev()`, lsm_tree.rs:692-696) — the     */
/* highest run index wins regardless of timestamp. Tombstones are     */
/* reported as found with value_len 0 so the caller distinguishes     */
/* deleted from absent (tests/db_server.rs delete->get->KeyNotFound   */
/* semantics). Bloom prefiltering stays on the host                   */
/* (dbeel_bloom_contains).                                            */
/* ------------------------------------------------------------------ */

__global__ void k_lookup(RunsDesc R, const uint8_t* keys,
                         const uint64_t* key_off, uint64_t n_keys,
                         dbeel_lookup_hit* out) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         q < n_keys; q += stride) {
        const uint8_t* key = keys + key_off[q];
        uint64_t klen = key_off[q + 1] - key_off[q];
        int best_run = -1;
        uint64_t best_off = 0, best_vlen = 0;
        /* newest-index-first, first match wins (lsm_tree.rs:692-696) */
        for (int r = R.n_runs - 1; r >= 0; r--) {
            uint64_t lo = blob_lower_bound(R, r, 0, R.count[r], key, klen);
            if (lo >= R.count[r]) continue;
            EView m;
            if (!load_entry(R, r, lo, m)) continue;
            if (m.klen != klen || cmp_keys(m.key, m.klen, key, klen) != 0)
                continue;
            best_run = r;
            best_off = m.off + 16 + m.klen; /* value bytes start */
            best_vlen = (uint64_t)m.full_size - 32 - m.klen;
            break;
        }
        out[q].run = best_run;
        out[q].is_tombstone = (best_run >= 0 && best_vlen == 0) ? 1 : 0;
        out[q].value_offset = best_off;
        out[q].value_len = best_vlen;
    }
}

extern "C" int dbeel_gpu_lookup(const dbeel_run_view* runs, size_t n_runs,
                                const uint8_t* keys,
                                const uint64_t* key_offsets, uint64_t n_keys,
                                int device, dbeel_lookup_hit* out) {
    g_err[0] = 0;
    if (!out || (n_keys && (!keys || !key_offsets))) {
        set_err("lookup: null argument");
        return DBEEL_ERR_INVALID_ARG;
    }
    int rc = validate_runs(runs, n_runs);
    if (rc) return rc;
    rc = select_device(device);
    if (rc) return rc;
    if (n_keys == 0) return DBEEL_OK;

    dbeel_gpu_job* job = nullptr;
    rc = dbeel_gpu_job_create(runs, n_runs, device, &job);
    if (rc) return rc;

    uint64_t kbytes = key_offsets[n_keys];
    uint8_t* d_keys = nullptr;
    uint64_t* d_koff = nullptr;
    dbeel_lookup_hit* d_out = nullptr;
    hipError_t e = hipMalloc(&d_keys, kbytes ? kbytes : 1);
    if (e == hipSuccess) e = hipMalloc(&d_koff, (n_keys + 1) * 8);
    if (e == hipSuccess)
        e = hipMalloc(&d_out, n_keys * sizeof(dbeel_lookup_hit));
    if (e == hipSuccess && kbytes)
        e = hipMemcpyAsync(d_keys, keys, kbytes, hipMemcpyHostToDevice,
                           job->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_koff, key_offsets, (n_keys + 1) * 8,
                           hipMemcpyHostToDevice, job->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_lookup, dim3(pick_grid(n_keys, 256)), dim3(256),
                           0, job->stream, job->desc, d_keys, d_koff, n_keys,
                           d_out);
        e = hipMemcpyAsync(out, d_out, n_keys * sizeof(dbeel_lookup_hit),
                           hipMemcpyDeviceToHost, job->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(job->stream);
    if (e == hipSuccess) e = hipGetLastError();
    hipFree(d_keys);
    hipFree(d_koff);
    hipFree(d_out);
    dbeel_gpu_job_destroy(job);
    if (e != hipSuccess) {
        set_err("lookup failed: %s", hipGetErrorString(e));
        return DBEEL_ERR_HIP;
    }
    return DBEEL_OK;
}

/* ------------------------------------------------------------------ */
/* Resident table reader                                              */
/*                                                                    */
/* dbeel_gpu_lookup above answers one batch by building a whole       */
/* compaction job. The reader keeps what a read needs resident — per  */
/* run one table: the padded run bytes, one dense big-endian 8-byte   */
/* key prefix per entry and the run's "DBLM" filter bitmap — and      */
/* answers any number of batches against the table list:              */
/*   k_reader_prepare : open-time pass; k_prepare's checks (bounds,   */
/*                      bincode field cross-check, monotone offsets)  */
/*                      plus strict key order inside each run, and    */
/*                      the prefix array. No aux records.             */
/*   k_reader_search  : thread per query; runs newest-index-first     */
/*                      (lsm_tree.rs:692-696): filter check with      */
/*                      early out, lower bound over the run's dense   */
/*                      prefix slice (8 keys per 64-B line, top       */
/*                      levels cache-resident), then the equal-prefix */
/*                      range is resolved by binary search with full  */
/*                      key compares on the blob. A non-empty         */
/*                      memtable is searched the same way ahead of    */
/*                      the tables, in an instantiation of its own.   */
/*   rocPRIM scan     : value_len -> exclusive value offsets.         */
/*   k_reader_gather  : wave per hit, 8-B chunks, exact-length reads. */
/*   k_reader_gather_entries : get_entries' gather (further down):    */
/*                      data_len | data | timestamp per hit,          */
/*                      tombstones included.                          */
/*   k_reader_adopt  : a compaction output copied device-to-device   */
/*                      into a new table gets its prefixes and filter */
/*                      bits in one pass (no validation: the engine   */
/*                      just wrote it).                               */
/* ------------------------------------------------------------------ */

struct ReaderBloom {
    const uint8_t* bits; /* device bitmap; NULL = run has no filter */
    uint64_t n_bits;
    uint64_t seed;
    uint32_t k;
    uint32_t rsv;
};

/* Per-run prefix arrays (each run is its own resident table). Passed by
 * value next to RunsDesc: 2.7 KiB + 0.5 KiB stays under the 4 KiB
 * kernel-argument limit. */
struct ReaderPfx {
    const uint64_t* p[MAX_RUNS];
};
/* The memtable as the search and gather kernels see it: one sorted run
 * with unique keys that the engine wrote itself (so its records are read
 * without the bounds checks of load_entry). count == 0 = empty: the search
 * then runs as the instantiation without the leg, and no hit names it for
 * the gather. It is not in RunsDesc — with 64
 * tables its position, n_runs, lies past the descriptor's arrays. */
struct ReaderMem {
    const uint8_t* data;
    const uint8_t* index;
    const uint64_t* pfx;
    uint64_t count;
};
static_assert(sizeof(ReaderMem) == 32, "memtable leg: 32 B of arguments");
static_assert(sizeof(RunsDesc) + sizeof(ReaderPfx) + sizeof(ReaderMem) + 64 <=
                  4096,
              "k_reader_search arguments must fit the kernarg segment");

/* stats slots of dbeel_get_stats, in order */
enum { RS_PROBES, RS_SKIPS, RS_SEARCHES, RS_HITS, RS_TOMBS, RS_N };

#define READER_BLOCK 256

__global__ void k_reader_prepare(RunsDesc R, uint64_t* pfx, uint32_t* err) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         g < R.total; g += stride) {
        int r = run_of(R, g);
        uint64_t i = g - R.entry_base[r];
        EView e;
        if (!load_entry(R, r, i, e)) {
            atomicOr(err, DERR_CORRUPT);
            pfx[g] = 0;
            continue;
        }
        pfx[g] = key_prefix(e.key, e.klen);
        if (!entry_consistent(R, r, i, e)) atomicOr(err, DERR_CORRUPT);
        /* the search depends on strictly ascending keys (flush invariant,
         * lsm_tree.rs:925-946); an invalid successor is flagged by its own
         * thread */
        EView nx;
        if (i + 1 < R.count[r] && load_entry(R, r, i + 1, nx) &&
            cmp_keys(e.key, e.klen, nx.key, nx.klen) >= 0)
            atomicOr(err, DERR_UNSORTED);
    }
}

/* The memtable leg of the search: the table loop's shape — bisect the
 * prefixes, then settle the equal-prefix stretch by bisection with full key
 * compares — over a run the engine wrote (its records are read without
 * load_entry's bounds checks). On a match off / vlen receive the value's
 * offset in the memtable's data and its length. */
__device__ __forceinline__ bool mem_search(const ReaderMem& M,
                                           const uint8_t* key, uint64_t klen,
                                           uint64_t qp, uint64_t& off,
                                           uint64_t& vlen) {
    uint64_t lo = pfx_lower_bound(M.pfx, M.count, qp);
    if (lo >= M.count || M.pfx[lo] != qp) return false;
    uint64_t end = lo + 1;
    if (end < M.count && M.pfx[end] == qp)
        end = pfx_upper_bound(M.pfx, end + 1, M.count, qp);
    while (lo < end) {
        const uint64_t mid = (lo + end) >> 1;
        const uint8_t* rec = M.index + mid * 16;
        const uint64_t eoff = ld_u64(rec);
        const uint64_t mklen = ld_u32(rec + 8) - 8;
        const int cmp = cmp_keys(M.data + eoff + 8, mklen, key, klen);
        if (cmp == 0) {
            off = eoff + 16 + mklen;
            vlen = (uint64_t)ld_u32(rec + 12) - 32 - mklen;
            return true;
        }
        if (cmp < 0)
            lo = mid + 1;
        else
            end = mid;
    }
    return false;
}

/* MEM = the memtable is not empty. With an empty one the launch takes the
 * <false> instantiation, whose code is the search without a memtable: the
 * get path does not pay for the feature until it is used. */
template <bool MEM>
__global__ __launch_bounds__(READER_BLOCK) void k_reader_search(
    RunsDesc R, ReaderPfx pfx, ReaderMem mem, const ReaderBloom* blooms,
    const uint8_t* keys, const uint64_t* key_off, uint64_t n_keys,
    dbeel_lookup_hit* out, unsigned long long* stats) {
    __shared__ unsigned long long s_stats[RS_N];
    if (threadIdx.x < RS_N) s_stats[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long c[RS_N] = {};
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         q < n_keys; q += stride) {
        const uint8_t* key = keys + key_off[q];
        uint64_t klen = key_off[q + 1] - key_off[q];
        const uint64_t qp = key_prefix(key, klen);
        /* hash pair of the filter seed last seen: filters written by
         * this engine share one seed, so it is computed once per query,
         * and only if a filtered run is reached */
        bool have_hash = false;
        uint64_t hseed = 0, h1 = 0, h2 = 0;
        int best_run = -1;
        uint64_t best_off = 0, best_vlen = 0;
        int r = R.n_runs - 1;
        /* a non-empty memtable is consulted before every table
         * (lsm_tree.rs:676-685) and counts as one visit to an unfiltered
         * run; a key found there is reported at the position a flush will
         * give it */
        if constexpr (MEM) {
            c[RS_SEARCHES]++;
            if (mem_search(mem, key, klen, qp, best_off, best_vlen)) {
                best_run = R.n_runs;
                r = -1;
            }
        }
        for (; r >= 0; r--) {
            const ReaderBloom B = blooms[r];
            if (B.bits) {
                c[RS_PROBES]++;
                if (!have_hash || hseed != B.seed) {
                    hseed = B.seed;
                    h1 = d_fnv1a64(key, klen, hseed);
                    h2 = d_fnv1a64(key, klen,
                                   hseed ^ 0x9e3779b97f4a7c15ull) | 1;
                    have_hash = true;
                }
                bool maybe = true;
                for (uint32_t j = 0; j < B.k; j++) {
                    uint64_t bit = (h1 + j * h2) % B.n_bits;
                    if (!(B.bits[bit >> 3] & (1u << (bit & 7)))) {
                        maybe = false;
                        break;
                    }
                }
                if (!maybe) {
                    c[RS_SKIPS]++;
                    continue;
                }
            }
            c[RS_SEARCHES]++;
            const uint64_t* P = pfx.p[r];
            const uint64_t n = R.count[r];
            uint64_t lo = pfx_lower_bound(P, n, qp);
            if (lo >= n || P[lo] != qp) continue;
            /* [lo, end) = entries sharing the query's prefix. Usually
             * one entry; otherwise its end is found by a second
             * bisection, never a walk */
            uint64_t end = lo + 1;
            if (end < n && P[end] == qp)
                end = pfx_upper_bound(P, end + 1, n, qp);
            /* equal prefixes are not equal keys (zero padding, length,
             * bytes past 8): the full compare on the blob decides. Keys
             * are unique inside a run, so a zero compare is the match and
             * ends the bisection with the entry in hand — which is why
             * this is not blob_lower_bound, whose answer would have to be
             * loaded and compared once more */
            bool found = false;
            EView m;
            while (lo < end) {
                uint64_t mid = (lo + end) >> 1;
                if (!load_entry(R, r, mid, m)) { /* validated at open */
                    end = mid;
                    continue;
                }
                int cmp = cmp_keys(m.key, m.klen, key, klen);
                if (cmp == 0) {
                    found = true;
                    break;
                }
                if (cmp < 0)
                    lo = mid + 1;
                else
                    end = mid;
            }
            if (!found) continue;
            best_run = r;
            best_off = m.off + 16 + m.klen; /* value bytes start */
            best_vlen = (uint64_t)m.full_size - 32 - m.klen;
            break;
        }
        if (best_run >= 0) {
            c[RS_HITS]++;
            if (best_vlen == 0) c[RS_TOMBS]++;
        }
        out[q].run = best_run;
        out[q].is_tombstone = (best_run >= 0 && best_vlen == 0) ? 1 : 0;
        out[q].value_offset = best_off;
        out[q].value_len = best_vlen;
    }
    #pragma unroll
    for (int s = 0; s < RS_N; s++)
        if (c[s]) atomicAdd(&s_stats[s], c[s]);
    __syncthreads();
    if (threadIdx.x < RS_N && s_stats[threadIdx.x])
        atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
}

struct HitValueLen {
    __device__ uint64_t operator()(const dbeel_lookup_hit& h) const {
        return h.value_len;
    }
};

/* One wave per query moves its value in 8-B chunks (byte tail by lane 0),
 * reading exactly value_len bytes — k_copy's staged span assumes >= 32-B
 * segments and cannot take 0/1-byte values. */
__global__ void k_reader_gather(RunsDesc R, const uint8_t* mem_data,
                                const dbeel_lookup_hit* hits,
                                const uint64_t* val_off, uint64_t n_keys,
                                uint8_t* values) {
    uint32_t lane = threadIdx.x & 63;
    uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t q = wave; q < n_keys; q += n_waves) {
        const dbeel_lookup_hit h = hits[q];
        if (h.run < 0 || h.value_len == 0) continue;
        /* run == n_runs names the memtable; with 64 tables that index lies
         * past R's arrays, so it is resolved before any of them is read */
        const uint8_t* src = h.run >= R.n_runs ? mem_data : R.data[h.run];
        wave_copy_bytes(values + val_off[q], src + h.value_offset,
                        h.value_len, lane);
    }
}

/* One resident run. d_run is laid out 16 B pad | data | index | 16 B pad:
 * the padding a job's input slab has, so a compaction job can borrow the
 * table as its input (k_copy's aligned loads may touch up to 15 B either
 * side of an entry). */
struct ReaderTable {
    uint8_t* d_run = nullptr;
    uint64_t* d_pfx = nullptr;  /* dense big-endian key prefixes         */
    uint8_t* d_bits = nullptr;  /* filter bitmap; NULL = run has none    */
    uint64_t data_len = 0, count = 0;
    ReaderBloom bloom{};        /* header fields; .bits == d_bits        */
    uint64_t bytes = 0;         /* requested bytes: run + prefixes + bitmap */
    /* holders of the three buffers: the list plus every snapshot scan that
     * reads them. NULL = the list alone (no snapshot has held the table
     * yet); allocated by the first snapshot, shared by every copy of this
     * struct, freed with the buffers by the last holder (table_free). */
    uint32_t* refs = nullptr;

    const uint8_t* data() const { return d_run + 16; }
    const uint8_t* index() const { return d_run + 16 + data_len; }
};

/* What a paged-scan page leaves on the device for the host's one read:
 * the copy's totals (st, read on-device by k_winmap / k_copy) plus where
 * the cursor goes. */
struct ScanPageTotals {
    StepTotals st;      /* bytes / entries TAKEN by the page; err unused   */
    uint64_t next;      /* window position of the first survivor not taken,
                           or the window length when all were taken        */
    uint64_t next_full; /* that survivor's full_size, 0 when there is none  */
    uint64_t shadowed;  /* NEWEST_ONLY: shadowed candidates among the first
                           `next`; not written by k_reader_scan_emit        */
};

struct dbeel_gpu_reader_scan;

/* A memtable buffer that snapshot scans read. While in_pair it is still one
 * of the ping-pong pair and counts in reserved_bytes; a put that would write
 * into it hands it over instead (in_pair = false, the pair takes a fresh
 * buffer) and it then lives, counted in held_bytes, until its last scan
 * ends. */
struct MemHold {
    uint8_t* d_run = nullptr;
    uint64_t* d_pfx = nullptr;
    uint64_t bytes = 0; /* run_cap + pfx_cap */
    uint32_t refs = 0;  /* scans */
    bool in_pair = true;
};

/* The resident memtable: one sorted run with unique keys in the table
 * layout (16 B pad | data | index | 16 B pad, plus the dense prefix array),
 * held in buf[cur]. A put builds its successor in buf[cur ^ 1] and swaps on
 * success, so a failed put leaves it untouched. The pair grows
 * geometrically and is kept across flush and clear; none of it counts in
 * table_bytes. A buffer that snapshot scans read (hold) is never written:
 * the put that would hands it over to them and puts a fresh one in its
 * place. */
struct ReaderMemtable {
    struct Buf {
        uint8_t* d_run = nullptr;
        uint64_t run_cap = 0; /* bytes */
        uint64_t* d_pfx = nullptr;
        uint64_t pfx_cap = 0; /* bytes */
        MemHold* hold = nullptr; /* set while snapshot scans read it */
    } buf[2];
    int cur = 0;
    uint64_t count = 0, data_len = 0, puts = 0;

    const uint8_t* data() const { return buf[cur].d_run + 16; }
    const uint8_t* index() const { return data() + data_len; }
    uint64_t reserved() const {
        return buf[0].run_cap + buf[0].pfx_cap + buf[1].run_cap +
               buf[1].pfx_cap;
    }
    ReaderMem view() const {
        if (!count) return ReaderMem{nullptr, nullptr, nullptr, 0};
        return ReaderMem{data(), index(), buf[cur].d_pfx, count};
    }
    void drop() { count = data_len = puts = 0; }
};

struct dbeel_gpu_reader {
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t ev[7] = {};
    /* the table list, in read-path order (highest position wins), and what
     * the kernels see of it — rebuilt by reader_link on every list edit */
    std::vector<ReaderTable> tables;
    RunsDesc desc{};
    ReaderPfx pfx{};
    ReaderBloom* d_blooms = nullptr; /* MAX_RUNS descriptors             */
    /* output of a compaction between begin and commit/abort; gets do not
     * see it */
    bool has_pending = false;
    ReaderTable pending;
    std::vector<uint32_t> pending_pos; /* its input tables, ascending    */
    /* puts not flushed yet; gets consult it before every table, scans see
     * it only when opened as snapshots with DBEEL_SCAN_MEMTABLE */
    ReaderMemtable mem;
    /* per-batch scratch, grown on demand and reused */
    uint8_t* d_keys = nullptr;
    uint64_t keys_cap = 0;
    uint8_t* d_batch = nullptr; /* key offsets | value offsets | hits */
    uint64_t batch_cap = 0;
    void* d_scantmp = nullptr;
    uint64_t scantmp_cap = 0;
    uint8_t* d_values = nullptr;
    uint64_t values_cap = 0;
    unsigned long long* d_stats = nullptr;
    /* get_merged, when this reader is the local one: candidates, winners,
     * offsets, merge hits and totals; the uploaded answers */
    uint8_t* d_merge = nullptr;
    uint64_t merge_cap = 0;
    uint8_t* d_answers = nullptr;
    uint64_t answers_cap = 0;
    /* paged scans: generation is bumped by every edit of the table list
     * (a scan from an older generation is stale); the per-page scratch, the
     * device page buffer and the copy's window map grow on demand and are
     * reused by every scan of this reader */
    uint64_t generation = 0;
    std::vector<dbeel_gpu_reader_scan*> scans;
    uint8_t* d_scan = nullptr;
    uint64_t scan_cap = 0;
    uint8_t* d_page = nullptr;
    uint64_t page_cap = 0;
    uint32_t* d_scanwin = nullptr;
    uint64_t scanwin_cap = 0;
    ScanPageTotals* d_scantot = nullptr;
    ScanPageTotals* h_scantot = nullptr; /* pinned */
};

static void reader_end_scans(dbeel_gpu_reader* rd);

static hipError_t reader_reserve(void** p, uint64_t* cap, uint64_t need) {
    if (need <= *cap) return hipSuccess;
    (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    uint64_t want = need + need / 4;
    hipError_t e = hipMalloc(p, want);
    if (e == hipSuccess) *cap = want;
    return e;
}

/* Lets go of one holder's reference; the last one frees the buffers. */
static void table_free(ReaderTable& t) {
    if (t.refs) {
        if (--*t.refs) {
            t = ReaderTable();
            return;
        }
        delete t.refs;
    }
    (void)hipFree(t.d_run);
    (void)hipFree(t.d_pfx);
    (void)hipFree(t.d_bits);
    t = ReaderTable();
}

/* bitmaps are whole 8-B words: k_reader_adopt sets bits through 4-B words */
static inline uint64_t bitmap_bytes(uint64_t n_bits) {
    return ((n_bits + 7) / 8 + 7) & ~7ull;
}

/* Right-sized allocations for one run; n_bits = 0 means no filter. On
 * failure t is left empty. */
static hipError_t table_alloc(ReaderTable& t, uint64_t data_len,
                              uint64_t count, uint64_t n_bits) {
    const uint64_t payload = data_len + count * 16;
    const uint64_t run_bytes = (payload ? payload : 16) + 32;
    const uint64_t pfx_bytes = (count ? count : 1) * sizeof(uint64_t);
    const uint64_t bm_bytes = n_bits ? bitmap_bytes(n_bits) : 0;
    t = ReaderTable();
    hipError_t e = hipMalloc(&t.d_run, run_bytes);
    if (e == hipSuccess) e = hipMalloc(&t.d_pfx, pfx_bytes);
    if (e == hipSuccess && bm_bytes) e = hipMalloc(&t.d_bits, bm_bytes);
    if (e != hipSuccess) {
        table_free(t);
        return e;
    }
    t.data_len = data_len;
    t.count = count;
    t.bytes = run_bytes + pfx_bytes + bm_bytes;
    return hipSuccess;
}

static RunsDesc table_desc(const ReaderTable& t) {
    RunsDesc D;
    memset(&D, 0, sizeof D);
    D.n_runs = 1;
    D.total = t.count;
    D.data[0] = t.data();
    D.index[0] = t.index();
    D.data_len[0] = t.data_len;
    D.count[0] = t.count;
    D.job_hi[0] = 1;
    return D;
}

/* Rebuilds the descriptors from the table list and uploads the filter
 * descriptors. The reader's stream is idle between calls, so nothing reads
 * d_blooms while it is rewritten. */
static hipError_t reader_link(dbeel_gpu_reader* rd) {
    ReaderBloom hb[MAX_RUNS];
    memset(hb, 0, sizeof hb);
    RunsDesc& D = rd->desc;
    memset(&D, 0, sizeof D);
    memset(&rd->pfx, 0, sizeof rd->pfx);
    D.n_runs = (int)rd->tables.size();
    uint64_t base = 0;
    for (size_t r = 0; r < rd->tables.size(); r++) {
        const ReaderTable& t = rd->tables[r];
        D.data[r] = t.data();
        D.index[r] = t.index();
        D.data_len[r] = t.data_len;
        D.count[r] = t.count;
        D.entry_base[r] = base;
        base += t.count;
        rd->pfx.p[r] = t.d_pfx;
        hb[r] = t.bloom;
        hb[r].bits = t.d_bits;
    }
    D.total = base;
    hipError_t e = hipMemcpyAsync(rd->d_blooms, hb, sizeof hb,
                                  hipMemcpyHostToDevice, rd->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(rd->stream);
    return e;
}

/* The list edit of every new table (insert_run, write_batch,
 * memtable_flush): t goes in at pos and the descriptor is linked again. On a
 * failed link the edit is undone, the old list linked back and t is still
 * the caller's to free. Once linked, open scans are stale (the generation
 * moves) and a pending compaction keeps naming the same tables. */
static hipError_t reader_insert_table(dbeel_gpu_reader* rd, size_t pos,
                                      const ReaderTable& t) {
    rd->tables.insert(rd->tables.begin() + pos, t);
    hipError_t e = reader_link(rd);
    if (e != hipSuccess) {
        rd->tables.erase(rd->tables.begin() + pos);
        (void)reader_link(rd);
        return e;
    }
    rd->generation++;
    for (uint32_t& p : rd->pending_pos)
        if (p >= pos) p++;
    return hipSuccess;
}

extern "C" void dbeel_gpu_reader_compact_abort(dbeel_gpu_reader* rd) {
    if (!rd || !rd->has_pending) return;
    if (rd->device >= 0) (void)hipSetDevice(rd->device);
    table_free(rd->pending);
    rd->pending_pos.clear();
    rd->has_pending = false;
}

extern "C" void dbeel_gpu_reader_close(dbeel_gpu_reader* rd) {
    if (!rd) return;
    if (rd->device >= 0) (void)hipSetDevice(rd->device);
    if (rd->stream) (void)hipStreamSynchronize(rd->stream);
    dbeel_gpu_reader_compact_abort(rd);
    reader_end_scans(rd);
    for (ReaderTable& t : rd->tables) table_free(t);
    for (ReaderMemtable::Buf& b : rd->mem.buf) {
        (void)hipFree(b.d_run);
        (void)hipFree(b.d_pfx);
    }
    (void)hipFree(rd->d_blooms);
    (void)hipFree(rd->d_keys);
    (void)hipFree(rd->d_batch);
    (void)hipFree(rd->d_scantmp);
    (void)hipFree(rd->d_values);
    (void)hipFree(rd->d_stats);
    (void)hipFree(rd->d_merge);
    (void)hipFree(rd->d_answers);
    (void)hipFree(rd->d_scan);
    (void)hipFree(rd->d_page);
    (void)hipFree(rd->d_scanwin);
    (void)hipFree(rd->d_scantot);
    if (rd->h_scantot) (void)hipHostFree(rd->h_scantot);
    for (int i = 0; i < 7; i++)
        if (rd->ev[i]) (void)hipEventDestroy(rd->ev[i]);
    if (rd->stream) (void)hipStreamDestroy(rd->stream);
    delete rd;
}

extern "C" uint64_t dbeel_gpu_reader_table_bytes(const dbeel_gpu_reader* rd) {
    if (!rd) return 0;
    uint64_t sum = rd->has_pending ? rd->pending.bytes : 0;
    for (const ReaderTable& t : rd->tables) sum += t.bytes;
    return sum;
}

extern "C" size_t dbeel_gpu_reader_run_count(const dbeel_gpu_reader* rd) {
    return rd ? rd->tables.size() : 0;
}

/* Library-internal (dbeel_lsm.cpp's bloom gate): data bytes of run pos. */
extern "C" uint64_t dbeel_reader_run_data_len(const dbeel_gpu_reader* rd, size_t pos) {
    return (rd && pos < rd->tables.size()) ? rd->tables[pos].data_len : 0;
}

/* "DBLM" header (include/dbeel_lsm.h): magic | ver | k | pad | n_bits |
 * seed, then the bitmap. Same acceptance rules as dbeel_bloom_contains. */
static int parse_bloom(const dbeel_bloom_view& v, size_t r,
                       ReaderBloom* out) {
    uint32_t ver, k;
    uint64_t n_bits, seed;
    if (v.len < 32 || memcmp(v.bytes, "DBLM", 4) != 0) {
        set_err("run %zu: filter is not a DBLM file", r);
        return DBEEL_ERR_CORRUPT;
    }
    memcpy(&ver, v.bytes + 4, 4);
    memcpy(&k, v.bytes + 8, 4);
    memcpy(&n_bits, v.bytes + 16, 8);
    memcpy(&seed, v.bytes + 24, 8);
    if (ver != 1) {
        set_err("run %zu: filter version %u unsupported", r, ver);
        return DBEEL_ERR_CORRUPT;
    }
    if (n_bits == 0) { /* the probe's modulus */
        set_err("run %zu: filter header declares zero bits", r);
        return DBEEL_ERR_CORRUPT;
    }
    if (n_bits > (uint64_t)(v.len - 32) * 8) {
        set_err("run %zu: filter of %zu bytes is shorter than its header's "
                "%llu bits", r, v.len, (unsigned long long)n_bits);
        return DBEEL_ERR_CORRUPT;
    }
    out->bits = nullptr;
    out->n_bits = n_bits;
    out->seed = seed;
    out->k = k;
    out->rsv = 0;
    return DBEEL_OK;
}

/* Allocates a table for one host run, enqueues its upload and the
 * k_reader_prepare pass over it (violations are OR-ed into *d_err) on the
 * reader's stream. hb = the run's parsed filter header, NULL = no filter.
 * The caller synchronises before the host buffers go away. */
static hipError_t reader_upload_table(dbeel_gpu_reader* rd,
                                      const dbeel_run_view& run,
                                      const dbeel_bloom_view* bloom,
                                      const ReaderBloom* hb, uint32_t* d_err,
                                      ReaderTable& t) {
    hipStream_t s = rd->stream;
    hipError_t e = table_alloc(t, run.data_len, run.index_len / 16,
                               hb ? hb->n_bits : 0);
    if (e != hipSuccess) return e;
    if (run.data_len)
        e = hipMemcpyAsync(t.d_run + 16, run.data, run.data_len,
                           hipMemcpyHostToDevice, s);
    if (e == hipSuccess && run.index_len)
        e = hipMemcpyAsync(t.d_run + 16 + run.data_len, run.index,
                           run.index_len, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && hb) {
        t.bloom = *hb;
        t.bloom.bits = t.d_bits;
        e = hipMemcpyAsync(t.d_bits, bloom->bytes + 32, (hb->n_bits + 7) / 8,
                           hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess && t.count)
        hipLaunchKernelGGL(k_reader_prepare, dim3(pick_grid(t.count, 256)),
                           dim3(256), 0, s, table_desc(t), t.d_pfx, d_err);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);
        table_free(t);
    }
    return e;
}

static void set_err_prepare(uint32_t err) {
    set_err(err & DERR_CORRUPT
                ? "corrupt input run (entry bounds/fields)"
                : "input run is not strictly ascending by key");
}

extern "C" int dbeel_gpu_reader_open(const dbeel_run_view* runs,
                                     const dbeel_bloom_view* blooms,
                                     size_t n_runs, int device,
                                     dbeel_gpu_reader** out_reader) {
    g_err[0] = 0;
    if (!out_reader) {
        set_err("reader_open: out is null");
        return DBEEL_ERR_INVALID_ARG;
    }
    *out_reader = nullptr;
    int rc = validate_runs(runs, n_runs);
    if (rc) return rc;
    rc = check_device_arg(device);
    if (rc) return rc;
    ReaderBloom hb[MAX_RUNS];
    memset(hb, 0, sizeof hb);
    for (size_t r = 0; r < n_runs; r++) {
        if (!blooms || !blooms[r].bytes) continue;
        rc = parse_bloom(blooms[r], r, &hb[r]);
        if (rc) return rc;
    }

    rc = select_device(device);
    if (rc) return rc;

    dbeel_gpu_reader* rd = new (std::nothrow) dbeel_gpu_reader();
    if (!rd) return DBEEL_ERR_OOM;
    ScopeGuard close_rd([&] { dbeel_gpu_reader_close(rd); });
    rd->device = device;

    uint32_t* d_err = nullptr;
    uint32_t err = 0;

    HIP_CHECK(hipStreamCreate(&rd->stream));
    for (int i = 0; i < 7; i++) HIP_CHECK(hipEventCreate(&rd->ev[i]));
    HIP_CHECK(hipMalloc(&rd->d_blooms, MAX_RUNS * sizeof(ReaderBloom)));
    HIP_CHECK(hipMalloc(&rd->d_stats, (RS_N + 1) * sizeof(uint64_t)));
    d_err = (uint32_t*)(rd->d_stats + RS_N);
    HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(uint64_t), rd->stream));
    rd->tables.reserve(MAX_RUNS);
    for (size_t r = 0; r < n_runs; r++) {
        const bool filtered = blooms && blooms[r].bytes;
        ReaderTable t;
        HIP_CHECK(reader_upload_table(rd, runs[r],
                                      filtered ? &blooms[r] : nullptr,
                                      filtered ? &hb[r] : nullptr, d_err, t));
        rd->tables.push_back(t);
    }
    HIP_CHECK(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost,
                             rd->stream));
    /* the caller's buffers are read by the async copies above */
    HIP_CHECK(hipStreamSynchronize(rd->stream));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(reader_link(rd));
    if (err) {
        set_err_prepare(err);
        return DBEEL_ERR_CORRUPT;
    }
    close_rd.dismiss();
    *out_reader = rd;
    return DBEEL_OK;
}

/* ---- Live updates: the shared sstable list of the reference's LSMTree
 * (flush pushes a table, lsm_tree.rs:901-915; compaction partitions out
 * its inputs, pushes the output and swaps the list while reads finish on
 * the old one, lsm_tree.rs:1113-1145). ---- */

extern "C" int dbeel_gpu_reader_insert_run(dbeel_gpu_reader* rd, size_t pos,
                                           const dbeel_run_view* run,
                                           const dbeel_bloom_view* bloom) {
    g_err[0] = 0;
    if (!rd || !run) {
        set_err("reader_insert_run: null argument");
        return DBEEL_ERR_INVALID_ARG;
    }
    if (pos > rd->tables.size()) {
        set_err("reader_insert_run: position %zu past the %zu runs held", pos,
                rd->tables.size());
        return DBEEL_ERR_INVALID_ARG;
    }
    if (rd->tables.size() >= MAX_RUNS) {
        set_err("reader_insert_run: reader already holds %d runs", MAX_RUNS);
        return DBEEL_ERR_INVALID_ARG;
    }
    int rc = validate_runs(run, 1);
    if (rc) return rc;
    const bool filtered = bloom && bloom->bytes;
    ReaderBloom hb;
    memset(&hb, 0, sizeof hb);
    if (filtered) {
        rc = parse_bloom(*bloom, pos, &hb);
        if (rc) return rc;
    }
    HIP_CHECK(hipSetDevice(rd->device));
    uint32_t* d_err = (uint32_t*)(rd->d_stats + RS_N);
    uint32_t err = 0;
    HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(uint64_t), rd->stream));
    ReaderTable t;
    hipError_t e = reader_upload_table(rd, *run, filtered ? bloom : nullptr,
                                       filtered ? &hb : nullptr, d_err, t);
    if (e == hipSuccess) {
        e = hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, rd->stream);
        hipError_t se = hipStreamSynchronize(rd->stream);
        if (e == hipSuccess) e = se;
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) table_free(t);
    }
    if (e != hipSuccess) {
        set_err("reader_insert_run: %s", hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? DBEEL_ERR_OOM : DBEEL_ERR_HIP;
    }
    if (err) {
        set_err_prepare(err);
        table_free(t);
        return DBEEL_ERR_CORRUPT;
    }
    e = reader_insert_table(rd, pos, t);
    if (e != hipSuccess) table_free(t);
    HIP_CHECK(e);
    return DBEEL_OK;
}

/* The device half of "fetch, re-upload, k_reader_prepare, k_bloom" for a
 * run the engine just produced (no validation): one pass over the index
 * records writes each entry's big-endian key prefix and, when bits is not
 * NULL, sets its k filter bits — dbeel_gpu_job_bloom's hash pair, so the
 * bitmap equals k_bloom's. Each key byte is read once and feeds the prefix
 * and both hashes. Bit positions are hash-scattered over the whole bitmap,
 * so the atomics see no systematic contention. */
__global__ void k_reader_adopt(const uint8_t* data, const uint8_t* index,
                               uint64_t n, uint64_t* pfx, uint32_t* bits,
                               uint64_t n_bits, uint64_t seed, uint32_t kk) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        const uint8_t* rec = index + i * 16;
        const uint8_t* key = data + ld_u64(rec) + 8;
        const uint64_t klen = ld_u32(rec + 8) - 8;
        if (!bits) {
            pfx[i] = key_prefix(key, klen);
            continue;
        }
        uint64_t v = 0;
        uint64_t h1 = 1469598103934665603ull ^ seed;
        uint64_t h2 = 1469598103934665603ull ^ seed ^ 0x9e3779b97f4a7c15ull;
        for (uint64_t j = 0; j < klen; j++) {
            const uint64_t c = key[j];
            if (j < 8) v |= c << (8 * j);
            h1 = (h1 ^ c) * 1099511628211ull;
            h2 = (h2 ^ c) * 1099511628211ull;
        }
        pfx[i] = __builtin_bswap64(v);
        h1 = d_mix64(h1);
        h2 = d_mix64(h2) | 1;
        for (uint32_t j = 0; j < kk; j++) {
            uint64_t bit = (h1 + j * h2) % n_bits;
            atomicOr(&bits[bit >> 5], 1u << (bit & 31));
        }
    }
}

/* Enqueues k_reader_adopt over a table whose run bytes are (being) written
 * on stream s: prefixes always, and with n_bits != 0 (the table was
 * allocated with that many) its zeroed-then-set filter bits. */
static hipError_t table_adopt(ReaderTable& t, uint64_t n_bits, hipStream_t s) {
    hipError_t e = hipSuccess;
    if (n_bits) {
        t.bloom.n_bits = n_bits;
        t.bloom.seed = BLOOM_SEED;
        t.bloom.k = BLOOM_K;
        t.bloom.bits = t.d_bits;
        e = hipMemsetAsync(t.d_bits, 0, bitmap_bytes(n_bits), s);
    }
    if (e == hipSuccess && t.count)
        hipLaunchKernelGGL(k_reader_adopt, dim3(pick_grid(t.count, 256)),
                           dim3(256), 0, s, t.data(), t.index(), t.count,
                           t.d_pfx, (uint32_t*)t.d_bits, n_bits,
                           (uint64_t)BLOOM_SEED, BLOOM_K);
    return e;
}

/* A table's filter as the "DBLM" file dbeel_gpu_job_bloom returns for the
 * same run: magic | ver | k | pad | n_bits | seed | bitmap. Engine-allocated
 * (dbeel_gpu_bloom_free); synchronises s. */
static int table_bloom_fetch(const ReaderTable& t, hipStream_t s,
                             uint8_t** out_bytes, uint64_t* out_len) {
    const uint64_t n_bits = t.bloom.n_bits;
    const uint64_t blen = 32 + (n_bits + 7) / 8;
    uint8_t* buf = (uint8_t*)calloc(1, blen + 4);
    if (!buf) {
        set_err("host alloc failed");
        return DBEEL_ERR_OOM;
    }
    const uint32_t ver = 1, kk = t.bloom.k, pad = 0;
    memcpy(buf, "DBLM", 4);
    memcpy(buf + 4, &ver, 4);
    memcpy(buf + 8, &kk, 4);
    memcpy(buf + 12, &pad, 4);
    memcpy(buf + 16, &n_bits, 8);
    memcpy(buf + 24, &t.bloom.seed, 8);
    hipError_t e = hipMemcpyAsync(buf + 32, t.d_bits, (n_bits + 7) / 8,
                                  hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        free(buf);
        set_err("filter D2H failed: %s", hipGetErrorString(e));
        return DBEEL_ERR_HIP;
    }
    *out_bytes = buf;
    *out_len = blen;
    return DBEEL_OK;
}

extern "C" int dbeel_gpu_reader_compact_begin(
    dbeel_gpu_reader* rd, const uint32_t* positions, size_t n_positions,
    int keep_tombstones, int build_bloom, dbeel_compact_result* out,
    uint8_t** bloom_bytes, uint64_t* bloom_len,
    dbeel_reader_compact_stats* stats) {
    g_err[0] = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (out) memset(out, 0, sizeof *out);
    if (bloom_bytes) *bloom_bytes = nullptr;
    if (bloom_len) *bloom_len = 0;
    if (!rd || !positions || n_positions == 0) {
        set_err("reader_compact_begin: null reader or no positions");
        return DBEEL_ERR_INVALID_ARG;
    }
    if ((bloom_bytes == nullptr) != (bloom_len == nullptr)) {
        set_err("reader_compact_begin: bloom_bytes and bloom_len go together");
        return DBEEL_ERR_INVALID_ARG;
    }
    if (rd->has_pending) {
        set_err("reader_compact_begin: a compaction is already pending");
        return DBEEL_ERR_INVALID_ARG;
    }
    for (size_t i = 0; i < n_positions; i++)
        if (positions[i] >= rd->tables.size() ||
            (i && positions[i] <= positions[i - 1])) {
            set_err("reader_compact_begin: positions must be strictly "
                    "ascending and below %zu", rd->tables.size());
            return DBEEL_ERR_INVALID_ARG;
        }
    HIP_CHECK(hipSetDevice(rd->device));
    /* the job reads the tables on its own stream */
    HIP_CHECK(hipStreamSynchronize(rd->stream));

    dbeel_run_view views[MAX_RUNS];
    for (size_t i = 0; i < n_positions; i++) {
        const ReaderTable& t = rd->tables[positions[i]];
        views[i] = {t.data(), (size_t)t.data_len, t.index(),
                    (size_t)(t.count * 16)};
    }
    dbeel_gpu_job* job = nullptr;
    uint32_t one[1] = {(uint32_t)n_positions};
    int rc = job_create_impl(views, n_positions, one, 1, rd->device, &job,
                             /*borrowed=*/true);
    if (rc) return rc;
    uint64_t out_data_len = 0, out_entries = 0;
    dbeel_compact_timings pt;
    memset(&pt, 0, sizeof pt);
    rc = dbeel_gpu_job_run(job, keep_tombstones, &out_data_len, &out_entries,
                           &pt);
    if (rc) {
        dbeel_gpu_job_destroy(job);
        return rc;
    }

    /* output -> right-sized resident table, device to device */
    const uint64_t n_bits = build_bloom ? bloom_bits_for(out_entries) : 0;
    ReaderTable t;
    hipStream_t s = job->stream;
    hipError_t e = table_alloc(t, out_data_len, out_entries, n_bits);
    float adopt_ms = 0, d2h_ms = 0;
    uint64_t d2h_bytes = 0;
    if (e == hipSuccess) e = hipEventRecord(job->ev[0], s);
    if (e == hipSuccess && out_data_len)
        e = hipMemcpyAsync(t.d_run + 16, job->d_outdata, out_data_len,
                           hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && out_entries)
        e = hipMemcpyAsync(t.d_run + 16 + out_data_len, job->d_outindex,
                           out_entries * 16, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = table_adopt(t, n_bits, s);
    if (e == hipSuccess) e = hipEventRecord(job->ev[1], s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipEventElapsedTime(&adopt_ms, job->ev[0],
                                                 job->ev[1]);
    if (e != hipSuccess) {
        set_err("reader_compact_begin: %s", hipGetErrorString(e));
        rc = e == hipErrorOutOfMemory ? DBEEL_ERR_OOM : DBEEL_ERR_HIP;
        goto fail;
    }

    /* host copies: what the caller writes to .compact_data/_index/_bloom */
    if (out || (bloom_bytes && n_bits)) {
        (void)hipEventRecord(job->ev[2], s);
        if (out) {
            rc = dbeel_gpu_job_fetch(job, out);
            if (rc) goto fail;
            d2h_bytes += out->data_len + out->index_len;
        }
        if (bloom_bytes && n_bits) {
            rc = table_bloom_fetch(t, s, bloom_bytes, bloom_len);
            if (rc) goto fail;
            d2h_bytes += (n_bits + 7) / 8;
        }
        (void)hipEventRecord(job->ev[3], s);
        (void)hipEventSynchronize(job->ev[3]);
        (void)hipEventElapsedTime(&d2h_ms, job->ev[2], job->ev[3]);
    }
    if (stats) {
        stats->pipeline = pt;
        stats->adopt_ms = adopt_ms;
        stats->d2h_ms = d2h_ms;
        stats->d2h_bytes = d2h_bytes;
        stats->entries_in = job->total_entries;
        stats->entries_out = out_entries;
        stats->data_bytes_out = out_data_len;
    }
    dbeel_gpu_job_destroy(job);
    rd->pending = t;
    rd->pending_pos.assign(positions, positions + n_positions);
    rd->has_pending = true;
    return DBEEL_OK;

fail:
    (void)hipStreamSynchronize(s);
    dbeel_gpu_job_destroy(job);
    table_free(t);
    if (out) dbeel_gpu_result_free(out);
    if (bloom_bytes && *bloom_bytes) {
        free(*bloom_bytes);
        *bloom_bytes = nullptr;
        *bloom_len = 0;
    }
    if (stats) memset(stats, 0, sizeof *stats);
    return rc;
}

extern "C" int dbeel_gpu_reader_compact_commit(dbeel_gpu_reader* rd,
                                               size_t out_pos) {
    g_err[0] = 0;
    if (!rd || !rd->has_pending) {
        set_err("reader_compact_commit: no compaction pending");
        return DBEEL_ERR_INVALID_ARG;
    }
    const size_t n_left = rd->tables.size() - rd->pending_pos.size();
    if (out_pos > n_left) {
        set_err("reader_compact_commit: out_pos %zu past the %zu runs left",
                out_pos, n_left);
        return DBEEL_ERR_INVALID_ARG;
    }
    HIP_CHECK(hipSetDevice(rd->device));
    /* one list edit: partition out the inputs, place the output */
    std::vector<ReaderTable> keep, gone;
    keep.reserve(MAX_RUNS);
    size_t k = 0;
    for (size_t r = 0; r < rd->tables.size(); r++) {
        if (k < rd->pending_pos.size() && rd->pending_pos[k] == r) {
            gone.push_back(rd->tables[r]);
            k++;
        } else {
            keep.push_back(rd->tables[r]);
        }
    }
    keep.insert(keep.begin() + out_pos, rd->pending);
    rd->tables.swap(keep);
    rd->generation++; /* open scans are stale from here on */
    rd->pending = ReaderTable();
    rd->pending_pos.clear();
    rd->has_pending = false;
    /* reader_link leaves the stream idle: nothing reads the old tables */
    hipError_t e = reader_link(rd);
    for (ReaderTable& t : gone) table_free(t);
    HIP_CHECK(e);
    return DBEEL_OK;
}

/* ------------------------------------------------------------------ */
/* Write batch: the memtable flush on the device                      */
/*                                                                    */
/* The reference's memtable is a red-black tree whose set() replaces  */
/* the value of an equal key whatever the timestamps are              */
/* (rbtree_arena/src/lib.rs:497-511); flush iterates it in key order  */
/* into EntryWriter and pushes the table onto the sstable list with   */
/* no bloom (lsm_tree.rs:882-915, 925-946). Here the writes arrive in */
/* arrival order, unsorted, with repeated keys:                       */
/*   k_batch_prefix : per write, big-endian 8-B key prefix + arrival  */
/*                    index.                                          */
/*   order          : two paths, chosen by DBEEL_BATCH_ORDER (read on */
/*                    every call). "radix": stable rocPRIM radix sort */
/*                    on (prefix, arrival), then only the writes whose*/
/*                    prefix equals a neighbour's are compacted,      */
/*                    merge-sorted by (prefix, key bytes past 8 and   */
/*                    length, arrival) and scattered back — no walk,  */
/*                    nothing quadratic when every key shares its     */
/*                    first 8 bytes. "merge" (the default, the faster */
/*                    one as measured): one merge sort over all pairs */
/*                    with the same comparator.                       */
/*   k_batch_flag   : equal keys are now adjacent in arrival order;   */
/*                    the last of each group survives. Emits RankRecs */
/*                    so survivor_scans gives positions and offsets.  */
/*   k_batch_totals : {bytes, survivors} for the host's one read,     */
/*                    which sizes the output.                         */
/*   k_batch_encode : wave per survivor, gathered through the arrival */
/*                    index from the staged blobs straight into the   */
/*                    output (a new resident table's allocation, or a */
/*                    plain buffer), index records included.          */
/* ------------------------------------------------------------------ */

struct BatchIn {
    uint64_t n;
    const uint8_t* keys;
    const uint64_t* koff;
    const uint8_t* vals;
    const uint64_t* voff;
    const uint8_t* ts;
};

/* One (prefix, arrival) pair as the merge sort moves it. */
struct BatchPair {
    uint64_t pfx;
    uint32_t arr;
    uint32_t rsv;
};

/* Where the keys lie, for compares by arrival index: the staged key blob
 * addressed through koff (index == NULL), or a page of run-format entries
 * (keys = its data, index = its 16-B records; key a at keys + off + 8 with
 * key_size - 8 bytes — every record passed k_page_stage). n bounds the
 * arrival indices. */
struct BatchKeys {
    const uint8_t* keys;
    const uint64_t* koff;
    uint32_t n;
    const uint8_t* index;
};

/* The one accessor both input shapes share. */
__device__ __forceinline__ const uint8_t* batch_key(const BatchKeys& K,
                                                    uint32_t a,
                                                    uint64_t& klen) {
    if (K.index) {
        const uint8_t* rec = K.index + (uint64_t)a * 16;
        klen = ld_u32(rec + 8) - 8;
        return K.keys + ld_u64(rec) + 8;
    }
    const uint64_t o = K.koff[a];
    klen = K.koff[a + 1] - o;
    return K.keys + o;
}

/* Order of two writes whose 8-byte prefixes are EQUAL: when both keys are
 * longer than 8 bytes, cmp_keys on the bytes past them; otherwise the
 * shorter key is a prefix of the other (the prefix is zero-padded), so the
 * lengths decide. */
__device__ __forceinline__ int batch_cmp_tied(const BatchKeys& K, uint32_t a,
                                              uint32_t b) {
    uint64_t la, lb;
    const uint8_t* ka = batch_key(K, a, la);
    const uint8_t* kb = batch_key(K, b, lb);
    if (la > 8 && lb > 8) return cmp_keys(ka + 8, la - 8, kb + 8, lb - 8);
    return la < lb ? -1 : (la > lb ? 1 : 0);
}

/* prefix, then key, then arrival. A pair whose arrival index is not below
 * n is no write of this batch (a sort may hand the comparator padding): it
 * is never dereferenced and orders after every real pair. */
struct BatchLess {
    BatchKeys K;
    __device__ bool operator()(const BatchPair& a, const BatchPair& b) const {
        if (a.arr >= K.n || b.arr >= K.n) return a.arr < b.arr;
        if (a.pfx != b.pfx) return a.pfx < b.pfx;
        const int c = batch_cmp_tied(K, a.arr, b.arr);
        return c ? c < 0 : a.arr < b.arr;
    }
};

__global__ void k_batch_prefix(BatchKeys K, uint64_t* pfx, uint32_t* arr) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < K.n;
         i += stride) {
        uint64_t klen;
        const uint8_t* key = batch_key(K, i, klen);
        pfx[i] = key_prefix(key, klen);
        arr[i] = i;
    }
}

/* tie[i] = 1 iff sorted prefix i equals a neighbour's. */
__global__ void k_batch_tieflag(uint32_t n, const uint64_t* pfx,
                                uint32_t* tie) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        const uint64_t p = pfx[i];
        tie[i] = ((i && pfx[i - 1] == p) || (i + 1 < n && pfx[i + 1] == p))
                     ? 1u : 0u;
    }
}

/* Gathers the flagged (tie == NULL: all) pairs into a dense list, and puts
 * a sorted list back into the same positions in ascending order. */
__global__ void k_batch_pairs(uint32_t n, const uint64_t* pfx,
                              const uint32_t* arr, const uint32_t* tie,
                              const uint32_t* tpos, BatchPair* out) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        if (tie && !tie[i]) continue;
        BatchPair p = {pfx[i], arr[i], 0};
        out[tie ? tpos[i] : i] = p;
    }
}

__global__ void k_batch_unpairs(uint32_t n, const BatchPair* in,
                                const uint32_t* tie, const uint32_t* tpos,
                                uint64_t* pfx, uint32_t* arr) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        if (tie && !tie[i]) continue;
        const BatchPair p = in[tie ? tpos[i] : i];
        pfx[i] = p.pfx;
        arr[i] = p.arr;
    }
}

/* Sorted write i of n survives iff it is the last one or its key differs
 * from its successor's (equal keys are adjacent, in arrival order: the last
 * arrival wins). src = keep flag | arrival index. full_size is what the
 * encode will write: from voff for the arrays, the page record's own for a
 * page, and 32 + klen for a page applied as tombstones. */
__global__ void k_batch_flag(BatchKeys K, uint32_t n, const uint64_t* pfx,
                             const uint32_t* arr, const uint64_t* voff,
                             int tomb, RankRec* rrec) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        const uint32_t a = arr[i];
        uint64_t klen;
        (void)batch_key(K, a, klen);
        const bool keep = i + 1 == n || pfx[i] != pfx[i + 1] ||
                          batch_cmp_tied(K, a, arr[i + 1]) != 0;
        RankRec r;
        r.src = (keep ? RR_KEEP : 0) | a;
        r.key_size = (uint32_t)(8 + klen);
        if (!K.index)
            r.full_size = (uint32_t)(32 + klen + (voff[a + 1] - voff[a]));
        else if (tomb)
            r.full_size = (uint32_t)(32 + klen);
        else
            r.full_size = ld_u32(K.index + (uint64_t)a * 16 + 12);
        rrec[i] = r;
    }
}

__global__ void k_batch_totals(const RankRec* rrec, const uint64_t* dst_off,
                               const uint32_t* pos, uint32_t n,
                               const uint32_t* zero, StepTotals* tot) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
        store_totals(tot, zero, rrec[n - 1], dst_off[n - 1], pos[n - 1]);
}

__global__ void k_batch_encode(uint32_t n, const RankRec* rrec,
                               const uint64_t* dst_off, const uint32_t* pos,
                               const uint8_t* keys, const uint64_t* koff,
                               const uint8_t* vals, const uint64_t* voff,
                               const uint8_t* ts, uint8_t* out_data,
                               uint8_t* out_index) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t i = wave; i < n; i += n_waves) {
        const RankRec r = rrec[i];
        if (!(r.src & RR_KEEP)) continue;
        const uint32_t a = (uint32_t)r.src;
        const uint64_t klen = r.key_size - 8;
        const uint64_t vlen = (uint64_t)r.full_size - 32 - klen;
        const uint64_t off = dst_off[i];
        uint8_t* dst = out_data + off;
        if (lane == 0) {
            __builtin_memcpy(dst, &klen, 8);
            __builtin_memcpy(dst + 8 + klen, &vlen, 8);
            __builtin_memcpy(dst + 16 + klen + vlen, ts + (uint64_t)a * 16,
                             16);
            uint8_t* rec = out_index + (uint64_t)pos[i] * 16;
            __builtin_memcpy(rec, &off, 8);
            __builtin_memcpy(rec + 8, &r.key_size, 4);
            __builtin_memcpy(rec + 12, &r.full_size, 4);
        }
        wave_copy_bytes(dst + 8, keys + koff[a], klen, lane);
        wave_copy_bytes(dst + 16 + klen, vals + voff[a], vlen, lane);
    }
}

/* What both entry points ask of the arrays, on the host. */
static int batch_check_arrays(const char* who, const BatchIn& in) {
    if (in.n && (!in.keys || !in.koff || !in.vals || !in.voff || !in.ts)) {
        set_err("%s: null array", who);
        return DBEEL_ERR_INVALID_ARG;
    }
    return DBEEL_OK;
}

/* 2^31 writes or more (arrival indices and the kernels' loop counters are
 * u32, and a counter plus one grid stride must not wrap) and a descending
 * offset are DBEEL_ERR_INVALID_ARG at once; *too_large
 * receives the first write with 32 + klen + vlen > u32::MAX, n when there
 * is none (error.rs:60-61), for the caller to report after its own checks. */
static int batch_check_offsets(const char* who, const BatchIn& in,
                               uint64_t* too_large) {
    *too_large = in.n;
    if (in.n >= (1ull << 31)) {
        set_err("%s: %llu writes, at most 2^31 - 1 per batch", who,
                (unsigned long long)in.n);
        return DBEEL_ERR_INVALID_ARG;
    }
    for (uint64_t i = 0; i < in.n; i++) {
        if (in.koff[i + 1] < in.koff[i] || in.voff[i + 1] < in.voff[i]) {
            set_err("%s: offsets of write %llu descend", who,
                    (unsigned long long)i);
            return DBEEL_ERR_INVALID_ARG;
        }
        const uint64_t klen = in.koff[i + 1] - in.koff[i];
        const uint64_t vlen = in.voff[i + 1] - in.voff[i];
        if (*too_large == in.n && (klen > 0xFFFFFFFFull ||
                                   vlen > 0xFFFFFFFFull ||
                                   32 + klen + vlen > 0xFFFFFFFFull))
            *too_large = i;
    }
    return DBEEL_OK;
}

static int batch_too_large(const char* who, uint64_t i) {
    set_err("%s: write %llu is larger than u32::MAX bytes encoded", who,
            (unsigned long long)i);
    return DBEEL_ERR_ITEM_TOO_LARGE;
}

/* Device staging and scratch of ONE call; the call frees it. */
struct BatchStage {
    uint8_t* d_slab = nullptr;    /* everything sized by the input alone   */
    void* d_tmp = nullptr;        /* rocPRIM scratch: radix sort and scans */
    BatchPair* d_pairs = nullptr; /* merge sort: pairs in | pairs out      */
    void* d_mtmp = nullptr;       /* merge sort scratch                    */
    struct Host {
        StepTotals tot;
        uint32_t tie_pos, tie_flag; /* of the last write: their sum is the
                                       tied count */
        uint32_t err;               /* a page's stage: DERR_* bits */
    }* h = nullptr;               /* pinned                                */
    /* carved out of d_slab */
    uint8_t *keys, *vals, *ts;
    uint64_t *koff, *voff, *pfx[2];
    uint32_t *arr[2], *tie, *tpos, *zero;
    RankRec* rrec;
    StepTotals* tot;
    uint8_t* extra;               /* the caller's own piece                */
    size_t tmp_bytes = 0;         /* of d_tmp                              */
    int cur = 0;                  /* pfx[cur] / arr[cur] hold the order    */
    uint64_t* dst_off() const { return pfx[cur ^ 1]; } /* free after order */
    uint32_t* pos() const { return tie; }              /* free after order */
    BatchKeys K = {};             /* the key source; K.n bounds arrivals   */
    const uint8_t* d_dts = nullptr; /* a page applied as tombstones: their
                                       timestamp, 16 B on the device       */
    uint32_t n = 0;               /* writes ordered: K.n, or the page
                                     entries its mask selected             */
    uint64_t n_surv = 0, total_bytes = 0, prefix_tied = 0;
};

static void batch_release(BatchStage& b) {
    (void)hipFree(b.d_slab);
    (void)hipFree(b.d_tmp);
    (void)hipFree(b.d_pairs);
    (void)hipFree(b.d_mtmp);
    if (b.h) (void)hipHostFree(b.h);
    b = BatchStage();
}

/* merge-sorts m pairs of b.d_pairs[0..m) into b.d_pairs[m..2m). */
static int batch_merge_sort(BatchStage& b, uint64_t m, hipStream_t s) {
    const BatchLess less = {b.K};
    size_t bytes = 0;
    HIP_CHECK(rocprim::merge_sort(nullptr, bytes, b.d_pairs, b.d_pairs + m, m,
                                  less, s));
    HIP_CHECK(hipMalloc(&b.d_mtmp, bytes ? bytes : 1));
    HIP_CHECK(rocprim::merge_sort(b.d_mtmp, bytes, b.d_pairs, b.d_pairs + m,
                                  m, less, s));
    return DBEEL_OK;
}

/* The slab and the rocPRIM scratch for n writes: the arrays' staging
 * (kbytes of keys, vbytes of values; a page has no arrays and stages
 * nothing of them) plus `extra` bytes for the caller, at b.extra. */
static int batch_alloc(BatchStage& b, uint32_t n, bool arrays,
                       uint64_t kbytes, uint64_t vbytes, uint64_t extra,
                       hipStream_t s) {
    const uint64_t na = arrays ? n : 0; /* per-write array staging */
    /* the slab: 16-B aligned pieces */
    uint64_t at = 0;
    auto carve = [&](uint64_t bytes) {
        const uint64_t o = at;
        at += (bytes + 15) & ~15ull;
        return o;
    };
    const uint64_t o_keys = carve(kbytes), o_vals = carve(vbytes),
                   o_ts = carve(na * 16),
                   o_koff = carve(arrays ? (na + 1) * 8 : 0),
                   o_voff = carve(arrays ? (na + 1) * 8 : 0),
                   o_pfx0 = carve((uint64_t)n * 8),
                   o_pfx1 = carve((uint64_t)n * 8),
                   o_arr0 = carve((uint64_t)n * 4),
                   o_arr1 = carve((uint64_t)n * 4),
                   o_tie = carve((uint64_t)n * 4),
                   o_tpos = carve((uint64_t)n * 4),
                   o_rrec = carve((uint64_t)n * sizeof(RankRec)),
                   o_tot = carve(sizeof(StepTotals)), o_zero = carve(16),
                   o_extra = carve(extra);
    HIP_CHECK(hipMalloc(&b.d_slab, at));
    HIP_CHECK(hipHostMalloc(&b.h, sizeof *b.h));
    uint8_t* S = b.d_slab;
    b.keys = S + o_keys;
    b.vals = S + o_vals;
    b.ts = S + o_ts;
    b.koff = (uint64_t*)(S + o_koff);
    b.voff = (uint64_t*)(S + o_voff);
    b.pfx[0] = (uint64_t*)(S + o_pfx0);
    b.pfx[1] = (uint64_t*)(S + o_pfx1);
    b.arr[0] = (uint32_t*)(S + o_arr0);
    b.arr[1] = (uint32_t*)(S + o_arr1);
    b.tie = (uint32_t*)(S + o_tie);
    b.tpos = (uint32_t*)(S + o_tpos);
    b.rrec = (RankRec*)(S + o_rrec);
    b.tot = (StepTotals*)(S + o_tot);
    b.zero = (uint32_t*)(S + o_zero);
    b.extra = S + o_extra;

    /* one scratch buffer for the primitives whose size n alone decides */
    size_t t_radix = 0, t_scan = 0, t_surv = 0;
    HIP_CHECK(rocprim::radix_sort_pairs(nullptr, t_radix, b.pfx[0], b.pfx[1],
                                        b.arr[0], b.arr[1], n, 0, 64, s));
    HIP_CHECK(rocprim::exclusive_scan(nullptr, t_scan, b.tie, b.tpos,
                                      (uint32_t)0, n,
                                      rocprim::plus<uint32_t>(), s));
    HIP_CHECK(survivor_scans(nullptr, t_surv, b.rrec, b.pfx[0], b.tie, n, s));
    size_t tmp_bytes = t_radix > t_scan ? t_radix : t_scan;
    if (t_surv > tmp_bytes) tmp_bytes = t_surv;
    HIP_CHECK(hipMalloc(&b.d_tmp, tmp_bytes ? tmp_bytes : 1));
    b.tmp_bytes = tmp_bytes;
    return DBEEL_OK;
}

/* Steps 3-4 over the b.n writes whose prefixes and arrival indices lie in
 * b.pfx[0] / b.arr[0], keys read through b.K. bound = the most bytes the
 * survivors can come to. ev as batch_order's: ev[2] is recorded here. */
static int batch_sort_flag(BatchStage& b, int tomb, uint64_t bound,
                           hipStream_t s, hipEvent_t* ev) {
    const uint32_t n = b.n;
    const BatchKeys& K = b.K;
    const size_t tmp_bytes = b.tmp_bytes;
    /* measured: the single merge sort is the faster of
     * the two on three of the four benchmark shapes, so it is the default */
    const char* mode = getenv("DBEEL_BATCH_ORDER");
    const bool merge_all = !(mode && strcmp(mode, "radix") == 0);
    const dim3 grid(pick_grid(n, 256)), block(256);

    /* 3. order */
    if (merge_all) {
        HIP_CHECK(hipMalloc(&b.d_pairs, 2ull * n * sizeof(BatchPair)));
        hipLaunchKernelGGL(k_batch_pairs, grid, block, 0, s, n, b.pfx[0],
                           b.arr[0], (const uint32_t*)nullptr,
                           (const uint32_t*)nullptr, b.d_pairs);
        int rc = batch_merge_sort(b, n, s);
        if (rc) return rc;
        hipLaunchKernelGGL(k_batch_unpairs, grid, block, 0, s, n,
                           b.d_pairs + n, (const uint32_t*)nullptr,
                           (const uint32_t*)nullptr, b.pfx[0], b.arr[0]);
        b.cur = 0;
    } else {
        size_t tb = tmp_bytes;
        HIP_CHECK(rocprim::radix_sort_pairs(b.d_tmp, tb, b.pfx[0], b.pfx[1],
                                            b.arr[0], b.arr[1], n, 0, 64, s));
        b.cur = 1;
    }
    /* the equal-prefix stretches: flag, count (= prefix_tied) */
    uint64_t* pfx = b.pfx[b.cur];
    uint32_t* arr = b.arr[b.cur];
    hipLaunchKernelGGL(k_batch_tieflag, grid, block, 0, s, n, pfx, b.tie);
    {
        size_t tb = tmp_bytes;
        HIP_CHECK(rocprim::exclusive_scan(b.d_tmp, tb, b.tie, b.tpos,
                                          (uint32_t)0, n,
                                          rocprim::plus<uint32_t>(), s));
    }
    HIP_CHECK(hipMemcpyAsync(&b.h->tie_pos, b.tpos + (n - 1), 4,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&b.h->tie_flag, b.tie + (n - 1), 4,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    const uint64_t m = b.prefix_tied = (uint64_t)b.h->tie_pos + b.h->tie_flag;
    if (m > n) {
        set_err("write batch: tied count %llu exceeds the %u writes",
                (unsigned long long)m, n);
        return DBEEL_ERR_HIP;
    }
    if (m && !merge_all) {
        /* settle them: compact, merge sort, scatter back in place */
        HIP_CHECK(hipMalloc(&b.d_pairs, 2 * m * sizeof(BatchPair)));
        hipLaunchKernelGGL(k_batch_pairs, grid, block, 0, s, n, pfx, arr,
                           b.tie, b.tpos, b.d_pairs);
        int rc = batch_merge_sort(b, m, s);
        if (rc) return rc;
        hipLaunchKernelGGL(k_batch_unpairs, grid, block, 0, s, n,
                           b.d_pairs + m, b.tie, b.tpos, pfx, arr);
    }
    if (ev) HIP_CHECK(hipEventRecord(ev[2], s));

    /* 4. survivors: flags, positions, byte offsets, totals */
    hipLaunchKernelGGL(k_batch_flag, grid, block, 0, s, K, n, pfx, arr,
                       (const uint64_t*)b.voff, tomb, b.rrec);
    {
        size_t tb = tmp_bytes;
        HIP_CHECK(survivor_scans(b.d_tmp, tb, b.rrec, b.dst_off(), b.pos(), n,
                                 s));
    }
    hipLaunchKernelGGL(k_batch_totals, dim3(1), dim3(64), 0, s, b.rrec,
                       b.dst_off(), b.pos(), n, b.zero, b.tot);
    HIP_CHECK(hipMemcpyAsync(&b.h->tot, b.tot, sizeof(StepTotals),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    b.n_surv = b.h->tot.n_surv;
    b.total_bytes = b.h->tot.total_out;
    /* what the encode kernel's stores are bounded by */
    if (b.n_surv == 0 || b.n_surv > n ||
        b.total_bytes > bound ||
        b.total_bytes < 32 * b.n_surv) {
        set_err("write batch: survivor totals %llu entries / %llu bytes are "
                "impossible for %u writes", (unsigned long long)b.n_surv,
                (unsigned long long)b.total_bytes, n);
        return DBEEL_ERR_HIP;
    }
    return DBEEL_OK;
}

/* Steps 1-4 on stream s: upload, prefixes, order, survivor flags and
 * scans; returns with the stream idle and n_surv / total_bytes /
 * prefix_tied known to the host. ev (NULL or 3 events) receives the marks
 * start | uploaded | ordered. The input was validated: in.n in [1, 2^31). */
static int batch_order(BatchStage& b, const BatchIn& in, hipStream_t s,
                       hipEvent_t* ev) {
    const uint32_t n = b.n = (uint32_t)in.n;
    const uint64_t kbytes = in.koff[n], vbytes = in.voff[n];
    int rc = batch_alloc(b, n, true, kbytes, vbytes, 0, s);
    if (rc) return rc;

    /* 1. upload */
    if (ev) HIP_CHECK(hipEventRecord(ev[0], s));
    if (kbytes)
        HIP_CHECK(hipMemcpyAsync(b.keys, in.keys, kbytes,
                                 hipMemcpyHostToDevice, s));
    if (vbytes)
        HIP_CHECK(hipMemcpyAsync(b.vals, in.vals, vbytes,
                                 hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(b.ts, in.ts, (uint64_t)n * 16,
                             hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(b.koff, in.koff, (uint64_t)(n + 1) * 8,
                             hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(b.voff, in.voff, (uint64_t)(n + 1) * 8,
                             hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(b.zero, 0, 16, s));
    if (ev) HIP_CHECK(hipEventRecord(ev[1], s));

    /* 2. prefixes */
    b.K = {b.keys, b.koff, n, nullptr};
    hipLaunchKernelGGL(k_batch_prefix, dim3(pick_grid(n, 256)), dim3(256), 0,
                       s, b.K, b.pfx[0], b.arr[0]);
    return batch_sort_flag(b, 0, 32ull * n + kbytes + vbytes, s, ev);
}

/* ---- A page of run-format entries as the batch (put_entries) ---- */

#define DERR_RANGE 4u /* a range id the take mask has no slot for */

/* R = the page as one run. Per entry: the loader's bounds check and the
 * consistency check (nothing is read through an entry that fails either),
 * the key prefix, and the selection flag for the compaction that follows.
 * The host reads err before any later kernel runs, so no kernel follows a
 * rejected entry. */
__global__ void k_page_stage(RunsDesc R, const uint32_t* rids,
                             const uint8_t* take, uint32_t n_take,
                             uint64_t* pfx, uint32_t* sel, uint32_t* err) {
    const uint32_t n = (uint32_t)R.count[0];
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        EView e;
        uint64_t p = 0;
        uint32_t keep = 0;
        if (!load_entry(R, 0, i, e) || !entry_consistent(R, 0, i, e)) {
            atomicOr(err, DERR_CORRUPT);
        } else {
            p = key_prefix(e.key, e.klen);
            if (!rids) {
                keep = 1;
            } else {
                const uint32_t id = rids[i];
                if (id >= n_take)
                    atomicOr(err, DERR_RANGE);
                else
                    keep = take[id] ? 1u : 0u;
            }
        }
        pfx[i] = p;
        sel[i] = keep;
    }
}

/* The selected entries, dense and still in arrival order: (prefix, arrival
 * index) of entry i goes to slot spos[i]. Unselected entries end here. */
__global__ void k_page_compact(uint32_t n, const uint64_t* pfx,
                               const uint32_t* sel, const uint32_t* spos,
                               uint64_t* pfx_out, uint32_t* arr_out) {
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        if (!sel[i]) continue;
        const uint32_t o = spos[i];
        pfx_out[o] = pfx[i];
        arr_out[o] = i;
    }
}

/* Wave per survivor. PUT (dts == NULL): the entry's bytes verbatim, one
 * copy of full_size bytes — nothing is taken apart. DELETE: klen | key |
 * 0 | dts, 32 + klen bytes (the size k_batch_flag scanned). Both write the
 * survivor's index record. */
__global__ void k_page_encode(uint32_t n, const RankRec* rrec,
                              const uint64_t* dst_off, const uint32_t* pos,
                              const uint8_t* data, const uint8_t* index,
                              const uint8_t* dts, uint8_t* out_data,
                              uint8_t* out_index) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t i = wave; i < n; i += n_waves) {
        const RankRec r = rrec[i];
        if (!(r.src & RR_KEEP)) continue;
        const uint32_t a = (uint32_t)r.src;
        const uint8_t* src = data + ld_u64(index + (uint64_t)a * 16);
        const uint64_t off = dst_off[i];
        uint8_t* dst = out_data + off;
        if (!dts) {
            wave_copy_bytes(dst, src, r.full_size, lane);
        } else {
            const uint64_t klen = r.key_size - 8, zero = 0;
            wave_copy_bytes(dst + 8, src + 8, klen, lane);
            if (lane == 0) {
                __builtin_memcpy(dst, &klen, 8);
                __builtin_memcpy(dst + 8 + klen, &zero, 8);
                __builtin_memcpy(dst + 16 + klen, dts, 16);
            }
        }
        if (lane == 0) {
            uint8_t* rec = out_index + (uint64_t)pos[i] * 16;
            __builtin_memcpy(rec, &off, 8);
            __builtin_memcpy(rec + 8, &r.key_size, 4);
            __builtin_memcpy(rec + 12, &r.full_size, 4);
        }
    }
}

/* 5. encode into out_data (total_bytes) / out_index (n_surv records). */
static void batch_encode(const BatchStage& b, hipStream_t s,
                         uint8_t* out_data, uint8_t* out_index) {
    if (b.K.index) {
        hipLaunchKernelGGL(k_page_encode,
                           dim3(pick_grid((uint64_t)b.n * 64, 256)), dim3(256),
                           0, s, b.n, b.rrec, b.dst_off(), b.pos(), b.K.keys,
                           b.K.index, b.d_dts, out_data, out_index);
        return;
    }
    hipLaunchKernelGGL(k_batch_encode,
                       dim3(pick_grid((uint64_t)b.n * 64, 256)), dim3(256), 0,
                       s, b.n, b.rrec, b.dst_off(), b.pos(), b.keys, b.koff,
                       b.vals, b.voff, b.ts, out_data, out_index);
}

/* Engine-allocated host copy of a run lying on the device; synchronises s.
 * On failure out is left zeroed. */
static int batch_fetch(const uint8_t* d_data, uint64_t dlen,
                       const uint8_t* d_index, uint64_t n_entries,
                       hipStream_t s, dbeel_compact_result* out) {
    const uint64_t ilen = n_entries * 16;
    ScopeGuard drop([&] { dbeel_gpu_result_free(out); });
    out->data = (uint8_t*)malloc(dlen ? dlen : 1);
    out->index = (uint8_t*)malloc(ilen ? ilen : 1);
    if (!out->data || !out->index) {
        set_err("host malloc failed");
        return DBEEL_ERR_OOM;
    }
    if (dlen)
        HIP_CHECK(hipMemcpyAsync(out->data, d_data, dlen,
                                 hipMemcpyDeviceToHost, s));
    if (ilen)
        HIP_CHECK(hipMemcpyAsync(out->index, d_index, ilen,
                                 hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    out->data_len = dlen;
    out->index_len = ilen;
    out->entries_written = n_entries;
    drop.dismiss();
    return DBEEL_OK;
}

extern "C" int dbeel_gpu_flush_batch(uint64_t n_writes, const uint8_t* keys,
                                     const uint64_t* key_offsets,
                                     const uint8_t* values,
                                     const uint64_t* value_offsets,
                                     const uint8_t* timestamps, int device,
                                     dbeel_compact_result* out) {
    g_err[0] = 0;
    if (!out) {
        set_err("flush_batch: out is null");
        return DBEEL_ERR_INVALID_ARG;
    }
    memset(out, 0, sizeof *out);
    const BatchIn in = {n_writes, keys, key_offsets, values, value_offsets,
                        timestamps};
    int rc = batch_check_arrays("flush_batch", in);
    if (rc) return rc;
    rc = check_device_arg(device);
    if (rc) return rc;
    uint64_t too_large = 0;
    rc = batch_check_offsets("flush_batch", in, &too_large);
    if (rc) return rc;
    if (too_large != in.n) return batch_too_large("flush_batch", too_large);
    if (in.n == 0) return DBEEL_OK; /* an empty memtable flushes nothing */
    rc = select_device(device);
    if (rc) return rc;

    BatchStage b;
    hipStream_t s = nullptr;
    uint8_t* d_out = nullptr;
    ScopeGuard release([&] {
        if (s) (void)hipStreamSynchronize(s);
        batch_release(b);
        (void)hipFree(d_out);
        if (s) (void)hipStreamDestroy(s);
    });
    HIP_CHECK(hipStreamCreate(&s));
    rc = batch_order(b, in, s, nullptr);
    if (rc) return rc;
    HIP_CHECK(hipMalloc(&d_out, b.total_bytes + b.n_surv * 16));
    batch_encode(b, s, d_out, d_out + b.total_bytes);
    HIP_CHECK(hipGetLastError());
    return batch_fetch(d_out, b.total_bytes, d_out + b.total_bytes, b.n_surv,
                       s, out);
}

extern "C" int dbeel_gpu_reader_write_batch(
    dbeel_gpu_reader* rd, size_t pos, uint64_t n_writes, const uint8_t* keys,
    const uint64_t* key_offsets, const uint8_t* values,
    const uint64_t* value_offsets, const uint8_t* timestamps, int build_bloom,
    dbeel_compact_result* out, uint8_t** bloom_bytes, uint64_t* bloom_len,
    dbeel_write_batch_stats* stats) {
    g_err[0] = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (out) memset(out, 0, sizeof *out);
    if (bloom_bytes) *bloom_bytes = nullptr;
    if (bloom_len) *bloom_len = 0;
    if (!rd) {
        set_err("reader_write_batch: null reader");
        return DBEEL_ERR_INVALID_ARG;
    }
    const BatchIn in = {n_writes, keys, key_offsets, values, value_offsets,
                        timestamps};
    int rc = batch_check_arrays("reader_write_batch", in);
    if (rc) return rc;
    if (pos > rd->tables.size()) {
        set_err("reader_write_batch: position %zu past the %zu runs held",
                pos, rd->tables.size());
        return DBEEL_ERR_INVALID_ARG;
    }
    if ((bloom_bytes == nullptr) != (bloom_len == nullptr)) {
        set_err("reader_write_batch: bloom_bytes and bloom_len go together");
        return DBEEL_ERR_INVALID_ARG;
    }
    uint64_t too_large = 0;
    rc = batch_check_offsets("reader_write_batch", in, &too_large);
    if (rc) return rc;
    if (in.n && rd->tables.size() >= MAX_RUNS) {
        set_err("reader_write_batch: reader already holds %d runs", MAX_RUNS);
        return DBEEL_ERR_INVALID_ARG;
    }
    if (too_large != in.n)
        return batch_too_large("reader_write_batch", too_large);
    if (in.n == 0) return DBEEL_OK; /* lsm_tree.rs:850-852 */

    HIP_CHECK(hipSetDevice(rd->device));
    hipStream_t s = rd->stream;
    BatchStage b;
    ReaderTable t;
    bool linked = false;
    ScopeGuard release([&] {
        (void)hipStreamSynchronize(s);
        batch_release(b);
        if (linked) return;
        table_free(t);
        if (out) dbeel_gpu_result_free(out);
        if (bloom_bytes && *bloom_bytes) {
            free(*bloom_bytes);
            *bloom_bytes = nullptr;
            *bloom_len = 0;
        }
    });
    rc = batch_order(b, in, s, rd->ev);
    if (rc) return rc;

    /* 5. encode straight into a right-sized table, 6. adopt it */
    const uint64_t n_bits = build_bloom ? bloom_bits_for(b.n_surv) : 0;
    HIP_CHECK(table_alloc(t, b.total_bytes, b.n_surv, n_bits));
    batch_encode(b, s, t.d_run + 16, t.d_run + 16 + b.total_bytes);
    HIP_CHECK(hipEventRecord(rd->ev[3], s));
    HIP_CHECK(table_adopt(t, n_bits, s));
    HIP_CHECK(hipEventRecord(rd->ev[4], s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());

    /* host copies: what the caller writes to {index}.data/.index/.bloom */
    uint64_t d2h_bytes = 0;
    const bool fetched = out || (bloom_bytes && n_bits);
    if (fetched) {
        HIP_CHECK(hipEventRecord(rd->ev[5], s));
        if (out) {
            rc = batch_fetch(t.data(), t.data_len, t.index(), t.count, s, out);
            if (rc) return rc;
            d2h_bytes += out->data_len + out->index_len;
        }
        if (bloom_bytes && n_bits) {
            rc = table_bloom_fetch(t, s, bloom_bytes, bloom_len);
            if (rc) return rc;
            d2h_bytes += (n_bits + 7) / 8;
        }
        HIP_CHECK(hipEventRecord(rd->ev[6], s));
        HIP_CHECK(hipEventSynchronize(rd->ev[6]));
    }
    dbeel_write_batch_stats st;
    memset(&st, 0, sizeof st);
    float ms[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++)
        HIP_CHECK(hipEventElapsedTime(&ms[i], rd->ev[i], rd->ev[i + 1]));
    if (fetched)
        HIP_CHECK(hipEventElapsedTime(&ms[4], rd->ev[5], rd->ev[6]));
    st.h2d_ms = ms[0];
    st.order_ms = ms[1];
    st.encode_ms = ms[2];
    st.adopt_ms = ms[3];
    st.d2h_ms = ms[4];
    st.writes_in = b.n;
    st.entries_out = b.n_surv;
    st.data_bytes_out = b.total_bytes;
    st.prefix_tied = b.prefix_tied;
    st.d2h_bytes = d2h_bytes;

    hipError_t e = reader_insert_table(rd, pos, t);
    HIP_CHECK(e); /* the guard above frees t */
    linked = true;
    if (stats) *stats = st;
    return DBEEL_OK;
}

/* Library-internal (dbeel_lsm.cpp: a flush whose files could not be
 * written): takes the table at pos out of the list again — the inverse of
 * reader_insert_table. */
extern "C" int dbeel_reader_drop_run(dbeel_gpu_reader* rd, size_t pos) {
    if (!rd || pos >= rd->tables.size()) return DBEEL_ERR_INVALID_ARG;
    HIP_CHECK(hipSetDevice(rd->device));
    HIP_CHECK(hipStreamSynchronize(rd->stream));
    ReaderTable t = rd->tables[pos];
    rd->tables.erase(rd->tables.begin() + pos);
    rd->generation++;
    for (uint32_t& p : rd->pending_pos)
        if (p > pos) p--;
    hipError_t e = reader_link(rd);
    table_free(t);
    HIP_CHECK(e);
    return DBEEL_OK;
}

/* ------------------------------------------------------------------ */
/* Resident memtable (include/dbeel_gpu.h): puts visible to gets,     */
/* flushed as one run                                                 */
/*                                                                    */
/* A put orders its batch with the write-batch stages (batch_order,   */
/* batch_encode) into a temporary run B, then merges B into the       */
/* memtable M, B winning equal keys — the rbtree's set() across       */
/* batches (rbtree_arena/src/lib.rs:497-511):                         */
/*   k_mem_rank : thread per entry of M and of B. Each bisects the    */
/*                OTHER run (prefix array, then the equal-prefix      */
/*                stretch with full key compares — never a walk) for  */
/*                its lower bound, which added to its own index is    */
/*                its slot in the merged order; an M entry whose key  */
/*                B holds is written without the keep flag. The slots */
/*                are a permutation of [0, m + b).                    */
/*   survivor_scans, k_emit, k_winmap, k_copy : the compaction's own  */
/*                tail over the two-run descriptor {M, B}, verbatim   */
/*                entry copy into the spare buffer.                   */
/*   k_reader_adopt : the merged prefix array.                        */
/* ------------------------------------------------------------------ */

struct MemPfx {
    const uint64_t* p[2];
};

/* Lower bound of (key, klen) in run r of R, whose n entries have the
 * prefixes P; eq = whether the entry there has that very key. */
__device__ __forceinline__ uint64_t mem_lower_bound(const RunsDesc& R, int r,
                                                    const uint64_t* P,
                                                    uint64_t qp,
                                                    const uint8_t* key,
                                                    uint64_t klen, bool& eq) {
    const uint64_t n = R.count[r];
    const uint64_t lo = pfx_lower_bound(P, n, qp);
    const uint64_t end = pfx_upper_bound(P, lo, n, qp);
    const uint64_t lb = blob_lower_bound(R, r, lo, end, key, klen);
    eq = false;
    EView m;
    if (lb < end && load_entry(R, r, lb, m))
        eq = cmp_keys(m.key, m.klen, key, klen) == 0;
    return lb;
}

/* R = {M, B}. Every slot is below R.total whatever the input holds (a
 * lower bound never exceeds the other run's count), so the store is in
 * bounds by construction; rrec is zeroed beforehand, so a slot nobody
 * claimed keeps nothing. */
__global__ void k_mem_rank(RunsDesc R, MemPfx pfx, RankRec* rrec,
                           uint32_t* err) {
    const uint64_t m = R.count[0];
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         g < R.total; g += stride) {
        const int r = g < m ? 0 : 1;
        const uint64_t i = r ? g - m : g;
        EView e;
        if (!load_entry(R, r, i, e)) { /* the engine wrote both runs */
            atomicOr(err, DERR_CORRUPT);
            continue;
        }
        bool eq;
        const uint64_t lb = mem_lower_bound(R, r ^ 1, pfx.p[r ^ 1], pfx.p[r][i],
                                            e.key, e.klen, eq);
        /* an equal pair: M's entry takes the lower slot and is dropped */
        const uint64_t slot = i + lb + ((r && eq) ? 1 : 0);
        const bool keep = r || !eq;
        RankRec rec;
        rec.src = ((uint64_t)r << 48) | e.off | (keep ? RR_KEEP : 0);
        rec.key_size = e.key_size;
        rec.full_size = e.full_size;
        rrec[slot] = rec;
    }
}

/* Makes buf hold a run of run_bytes and n prefixes; grows geometrically.
 * The buffer's old contents are not kept: it is the spare. */
static hipError_t mem_reserve(ReaderMemtable::Buf& buf, uint64_t run_bytes,
                              uint64_t n) {
    if (run_bytes > buf.run_cap) {
        const uint64_t want =
            run_bytes > 2 * buf.run_cap ? run_bytes : 2 * buf.run_cap;
        (void)hipFree(buf.d_run);
        buf.d_run = nullptr;
        buf.run_cap = 0;
        hipError_t e = hipMalloc(&buf.d_run, want);
        if (e != hipSuccess) return e;
        buf.run_cap = want;
    }
    const uint64_t pfx_bytes = (n ? n : 1) * sizeof(uint64_t);
    if (pfx_bytes > buf.pfx_cap) {
        const uint64_t want =
            pfx_bytes > 2 * buf.pfx_cap ? pfx_bytes : 2 * buf.pfx_cap;
        (void)hipFree(buf.d_pfx);
        buf.d_pfx = nullptr;
        buf.pfx_cap = 0;
        hipError_t e = hipMalloc(&buf.d_pfx, want);
        if (e != hipSuccess) return e;
        buf.pfx_cap = want;
    }
    return hipSuccess;
}

static inline uint64_t mem_run_bytes(uint64_t data_len, uint64_t count) {
    return data_len + count * 16 + 32;
}

/* What follows the order stage in every put: B (the ordered batch of b,
 * encoded by batch_encode for its input shape) merged into the memtable,
 * B winning equal keys, into the spare buffer; then the swap. rd->ev[0..2]
 * were recorded by the caller's stages on rd->stream; on failure nothing
 * of the memtable has changed. */
struct MemMerged {
    uint64_t batch_entries, replaced, entries, data_bytes;
    float ms[3]; /* ev[0]-[1] | ev[1]-[3] | ev[3]-[4] */
};

static int mem_merge(const char* who, dbeel_gpu_reader* rd, BatchStage& b,
                     MemMerged& out) {
    ReaderMemtable& M = rd->mem;
    hipStream_t s = rd->stream;
    uint8_t* d_brun = nullptr;   /* B: 16 B pad | data | index | 16 B pad */
    uint64_t* d_bpfx = nullptr;
    uint8_t* d_merge = nullptr;  /* the merge's scratch, carved below      */
    void* d_mtmp = nullptr;      /* its scans' rocPRIM scratch             */
    /* a spare that snapshot scans still read is not written: the new
     * memtable goes into a fresh buffer, and at the swap the held one is
     * handed over to its scans while the fresh one joins the pair. Until
     * then nothing has changed, so a failed put leaves every count as it
     * was. */
    ReaderMemtable::Buf fresh;
    const bool displace = M.buf[M.cur ^ 1].hold != nullptr;
    ScopeGuard release([&] {
        (void)hipStreamSynchronize(s);
        (void)hipFree(d_brun);
        (void)hipFree(d_bpfx);
        (void)hipFree(d_merge);
        (void)hipFree(d_mtmp);
        (void)hipFree(fresh.d_run);
        (void)hipFree(fresh.d_pfx);
    });

    const uint64_t m = M.count, nb = b.n_surv;
    ReaderMemtable::Buf& spare = displace ? fresh : M.buf[M.cur ^ 1];
    uint64_t new_count = 0, new_len = 0;
    if (m == 0) {
        /* nothing to merge with: the ordered batch is the memtable */
        HIP_CHECK(mem_reserve(spare, mem_run_bytes(b.total_bytes, nb), nb));
        batch_encode(b, s, spare.d_run + 16, spare.d_run + 16 + b.total_bytes);
        HIP_CHECK(hipEventRecord(rd->ev[3], s));
        hipLaunchKernelGGL(k_reader_adopt, dim3(pick_grid(nb, 256)), dim3(256),
                           0, s, spare.d_run + 16,
                           spare.d_run + 16 + b.total_bytes, nb, spare.d_pfx,
                           (uint32_t*)nullptr, (uint64_t)0, (uint64_t)0, 0u);
        HIP_CHECK(hipEventRecord(rd->ev[4], s));
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
        new_count = nb;
        new_len = b.total_bytes;
    } else {
        /* stage 1 ends: B as a padded temporary run with its prefixes */
        HIP_CHECK(hipMalloc(&d_brun, mem_run_bytes(b.total_bytes, nb)));
        HIP_CHECK(hipMalloc(&d_bpfx, nb * sizeof(uint64_t)));
        uint8_t* b_data = d_brun + 16;
        uint8_t* b_index = b_data + b.total_bytes;
        batch_encode(b, s, b_data, b_index);
        hipLaunchKernelGGL(k_reader_adopt, dim3(pick_grid(nb, 256)), dim3(256),
                           0, s, b_data, b_index, nb, d_bpfx,
                           (uint32_t*)nullptr, (uint64_t)0, (uint64_t)0, 0u);
        HIP_CHECK(hipEventRecord(rd->ev[3], s));

        /* stage 2: merge B into M */
        const uint64_t N = m + nb; /* < 2^31, checked above */
        const uint64_t in_bytes = M.data_len + b.total_bytes;
        RunsDesc D;
        memset(&D, 0, sizeof D);
        D.n_runs = 2;
        D.total = N;
        D.data[0] = M.data();
        D.index[0] = M.index();
        D.data_len[0] = M.data_len;
        D.count[0] = m;
        D.data[1] = b_data;
        D.index[1] = b_index;
        D.data_len[1] = b.total_bytes;
        D.count[1] = nb;
        D.entry_base[1] = m;
        D.job_hi[0] = D.job_hi[1] = 2;
        const MemPfx P = {{M.buf[M.cur].d_pfx, d_bpfx}};

        uint64_t at = 0;
        auto carve = [&](uint64_t bytes) {
            const uint64_t o = at;
            at += (bytes + 15) & ~15ull;
            return o;
        };
        /* the window map is sized for the smallest copy window (8 KiB) */
        const uint64_t o_rrec = carve(N * sizeof(RankRec)),
                       o_dst = carve(N * 8), o_pos = carve(N * 4),
                       o_oidx = carve(N * 16), o_smap = carve(N * 8),
                       o_win = carve((in_bytes / 8192 + 2) * 4),
                       o_tot = carve(sizeof(StepTotals)), o_err = carve(16);
        HIP_CHECK(hipMalloc(&d_merge, at));
        RankRec* d_rrec = (RankRec*)(d_merge + o_rrec);
        uint64_t* d_dst = (uint64_t*)(d_merge + o_dst);
        uint32_t* d_pos = (uint32_t*)(d_merge + o_pos);
        uint8_t* d_oidx = d_merge + o_oidx;
        uint64_t* d_smap = (uint64_t*)(d_merge + o_smap);
        uint32_t* d_win = (uint32_t*)(d_merge + o_win);
        StepTotals* d_tot = (StepTotals*)(d_merge + o_tot);
        uint32_t* d_err = (uint32_t*)(d_merge + o_err);
        size_t tmp_bytes = 0;
        HIP_CHECK(survivor_scans(nullptr, tmp_bytes, d_rrec, d_dst, d_pos, N,
                                 s));
        HIP_CHECK(hipMalloc(&d_mtmp, tmp_bytes ? tmp_bytes : 1));
        /* the spare is sized from the bound the totals are checked
         * against below */
        HIP_CHECK(mem_reserve(spare, mem_run_bytes(in_bytes, N), N));

        HIP_CHECK(hipMemsetAsync(d_rrec, 0, N * sizeof(RankRec), s));
        HIP_CHECK(hipMemsetAsync(d_tot, 0, o_err + 16 - o_tot, s));
        hipLaunchKernelGGL(k_mem_rank, dim3(pick_grid(N, 256)), dim3(256), 0,
                           s, D, P, d_rrec, d_err);
        HIP_CHECK(survivor_scans(d_mtmp, tmp_bytes, d_rrec, d_dst, d_pos, N,
                                 s));
        hipLaunchKernelGGL(k_emit, dim3(pick_grid(N, 256)), dim3(256), 0, s, D,
                           d_rrec, d_dst, d_pos, N, d_oidx, d_smap, d_err,
                           d_tot);
        HIP_CHECK(hipMemcpyAsync(&b.h->tot, d_tot, sizeof(StepTotals),
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
        new_count = b.h->tot.n_surv;
        new_len = b.h->tot.total_out;
        /* what the copy's stores are bounded by */
        if (b.h->tot.err || new_count > N || new_count < (m > nb ? m : nb) ||
            new_len > in_bytes || new_len < 32 * new_count) {
            set_err("%s: merge totals %llu entries / %llu bytes are "
                    "impossible for %llu + %llu entries (err %llu)",
                    who, (unsigned long long)new_count,
                    (unsigned long long)new_len, (unsigned long long)m,
                    (unsigned long long)nb,
                    (unsigned long long)b.h->tot.err);
            return DBEEL_ERR_HIP;
        }
        uint8_t* n_data = spare.d_run + 16;
        launch_copy(s, d_oidx, d_smap, d_win, d_tot, N, in_bytes, n_data);
        HIP_CHECK(hipMemcpyAsync(n_data + new_len, d_oidx, new_count * 16,
                                 hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_reader_adopt, dim3(pick_grid(new_count, 256)),
                           dim3(256), 0, s, n_data, n_data + new_len,
                           new_count, spare.d_pfx, (uint32_t*)nullptr,
                           (uint64_t)0, (uint64_t)0, 0u);
        HIP_CHECK(hipEventRecord(rd->ev[4], s));
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
    }
    float ms[3] = {0, 0, 0};
    HIP_CHECK(hipEventElapsedTime(&ms[0], rd->ev[0], rd->ev[1]));
    HIP_CHECK(hipEventElapsedTime(&ms[1], rd->ev[1], rd->ev[3]));
    HIP_CHECK(hipEventElapsedTime(&ms[2], rd->ev[3], rd->ev[4]));

    /* the swap: from here the new memtable answers */
    if (displace) {
        ReaderMemtable::Buf& old = M.buf[M.cur ^ 1];
        old.hold->bytes = old.run_cap + old.pfx_cap;
        old.hold->in_pair = false; /* its scans free it */
        old = fresh;
        fresh = ReaderMemtable::Buf();
    }
    M.cur ^= 1;
    M.count = new_count;
    M.data_len = new_len;
    M.puts++;
    out.batch_entries = nb;
    out.replaced = m + nb - new_count;
    out.entries = new_count;
    out.data_bytes = new_len;
    for (int i = 0; i < 3; i++) out.ms[i] = ms[i];
    return DBEEL_OK;
}

extern "C" int dbeel_gpu_reader_put(dbeel_gpu_reader* rd, uint64_t n_writes,
                                    const uint8_t* keys,
                                    const uint64_t* key_offsets,
                                    const uint8_t* values,
                                    const uint64_t* value_offsets,
                                    const uint8_t* timestamps,
                                    dbeel_memtable_put_stats* stats) {
    g_err[0] = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (!rd) {
        set_err("reader_put: null reader");
        return DBEEL_ERR_INVALID_ARG;
    }
    const BatchIn in = {n_writes, keys, key_offsets, values, value_offsets,
                        timestamps};
    int rc = batch_check_arrays("reader_put", in);
    if (rc) return rc;
    uint64_t too_large = 0;
    rc = batch_check_offsets("reader_put", in, &too_large);
    if (rc) return rc;
    ReaderMemtable& M = rd->mem;
    if (M.count + in.n >= (1ull << 31)) {
        set_err("reader_put: %llu memtable entries + %llu writes, at most "
                "2^31 - 1 together (flush first)",
                (unsigned long long)M.count, (unsigned long long)in.n);
        return DBEEL_ERR_INVALID_ARG;
    }
    if (too_large != in.n) return batch_too_large("reader_put", too_large);
    if (in.n == 0) return DBEEL_OK;

    HIP_CHECK(hipSetDevice(rd->device));
    hipStream_t s = rd->stream;
    BatchStage b;
    ScopeGuard release([&] {
        (void)hipStreamSynchronize(s);
        batch_release(b);
    });
    rc = batch_order(b, in, s, rd->ev);
    if (rc) return rc;
    MemMerged mm;
    rc = mem_merge("reader_put", rd, b, mm);
    if (rc) return rc;
    if (stats) {
        stats->h2d_ms = mm.ms[0];
        stats->order_ms = mm.ms[1];
        stats->merge_ms = mm.ms[2];
        stats->writes_in = b.n;
        stats->batch_entries = mm.batch_entries;
        stats->replaced = mm.replaced;
        stats->entries = mm.entries;
        stats->data_bytes = mm.data_bytes;
        stats->prefix_tied = b.prefix_tied;
    }
    return DBEEL_OK;
}

/* ------------------------------------------------------------------ */
/* Scan pages applied as puts or deletes (include/dbeel_gpu.h)         */
/*                                                                    */
/* The page replaces the five arrays as the batch's input:            */
/*   k_page_stage   : validates every entry, prefix + selection flag. */
/*   scan + k_page_compact : the selected entries, dense, in arrival  */
/*                    order — the unselected end before the sort.     */
/*   batch_sort_flag: the write batch's own order and survivor stages,*/
/*                    keys read in place through batch_key.           */
/*   k_page_encode  : wave per survivor, verbatim entry (PUT) or a    */
/*                    tombstone built from its key (DELETE).          */
/*   mem_merge      : what every put ends with.                       */
/* ------------------------------------------------------------------ */

struct PageIn {
    const uint8_t* data;
    uint64_t data_len;
    const uint8_t* index;
    uint64_t n;
    const uint32_t* rids; /* NULL = every entry selected */
    bool on_device;       /* the three lie on rd's device already */
};

/* The arguments passed the host checks: n in [1, 2^31), take / delete_ts
 * are host memory. */
static int put_entries_impl(const char* who, dbeel_gpu_reader* rd,
                            const PageIn& pg, const uint8_t* take,
                            uint32_t n_take, int mode,
                            const uint8_t* delete_ts,
                            dbeel_put_entries_stats* stats) {
    HIP_CHECK(hipSetDevice(rd->device));
    hipStream_t s = rd->stream;
    const uint32_t n = (uint32_t)pg.n;
    const int tomb = mode == DBEEL_APPLY_DELETE;
    BatchStage b;
    ScopeGuard release([&] {
        (void)hipStreamSynchronize(s);
        batch_release(b);
    });
    auto al16 = [](uint64_t v) { return (v + 15) & ~15ull; };
    const uint64_t o_take = 0, o_dts = o_take + al16(pg.rids ? n_take : 0),
                   o_err = o_dts + 16, o_data = o_err + 16,
                   o_index = o_data + (pg.on_device ? 0 : al16(pg.data_len)),
                   o_rids = o_index + (pg.on_device ? 0 : (uint64_t)n * 16),
                   extra = o_rids + ((pg.on_device || !pg.rids)
                                         ? 0 : al16((uint64_t)n * 4));
    int rc = batch_alloc(b, n, false, 0, 0, extra, s);
    if (rc) return rc;
    uint8_t* d_take = b.extra + o_take;
    uint8_t* d_dts = b.extra + o_dts;
    uint32_t* d_err = (uint32_t*)(b.extra + o_err);
    const uint8_t* d_data = pg.data;
    const uint8_t* d_index = pg.index;
    const uint32_t* d_rids = pg.rids;

    /* 1. upload: the mask and the timestamp; a host page into the slab */
    HIP_CHECK(hipEventRecord(rd->ev[0], s));
    if (!pg.on_device) {
        if (pg.data_len)
            HIP_CHECK(hipMemcpyAsync(b.extra + o_data, pg.data, pg.data_len,
                                     hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(b.extra + o_index, pg.index,
                                 (uint64_t)n * 16, hipMemcpyHostToDevice, s));
        d_data = b.extra + o_data;
        d_index = b.extra + o_index;
        if (pg.rids) {
            HIP_CHECK(hipMemcpyAsync(b.extra + o_rids, pg.rids,
                                     (uint64_t)n * 4, hipMemcpyHostToDevice,
                                     s));
            d_rids = (const uint32_t*)(b.extra + o_rids);
        }
    }
    HIP_CHECK(hipEventRecord(rd->ev[1], s));
    if (pg.rids)
        HIP_CHECK(hipMemcpyAsync(d_take, take, n_take, hipMemcpyHostToDevice,
                                 s));
    if (tomb)
        HIP_CHECK(hipMemcpyAsync(d_dts, delete_ts, 16, hipMemcpyHostToDevice,
                                 s));
    HIP_CHECK(hipMemsetAsync(d_err, 0, 16, s));
    HIP_CHECK(hipMemsetAsync(b.zero, 0, 16, s));

    /* 2. validate, prefixes, selection; the unselected are compacted away */
    RunsDesc D;
    memset(&D, 0, sizeof D);
    D.n_runs = 1;
    D.total = n;
    D.data[0] = d_data;
    D.index[0] = d_index;
    D.data_len[0] = pg.data_len;
    D.count[0] = n;
    D.job_hi[0] = 1;
    const dim3 grid(pick_grid(n, 256)), block(256);
    hipLaunchKernelGGL(k_page_stage, grid, block, 0, s, D, d_rids,
                       (const uint8_t*)d_take, n_take, b.pfx[1], b.tie,
                       d_err);
    {
        size_t tb = b.tmp_bytes;
        HIP_CHECK(rocprim::exclusive_scan(b.d_tmp, tb, b.tie, b.tpos,
                                          (uint32_t)0, n,
                                          rocprim::plus<uint32_t>(), s));
    }
    HIP_CHECK(hipMemcpyAsync(&b.h->tie_pos, b.tpos + (n - 1), 4,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&b.h->tie_flag, b.tie + (n - 1), 4,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&b.h->err, d_err, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    if (b.h->err & DERR_CORRUPT) {
        set_err("%s: corrupt page (an index record out of bounds, "
                "overlapping its successor, or disagreeing with the entry's "
                "length fields)", who);
        return DBEEL_ERR_CORRUPT;
    }
    if (b.h->err) {
        set_err("%s: a range id is not below n_take = %u", who, n_take);
        return DBEEL_ERR_INVALID_ARG;
    }
    const uint64_t n_sel = (uint64_t)b.h->tie_pos + b.h->tie_flag;
    if (n_sel > n) {
        set_err("%s: selected count %llu exceeds the %u entries", who,
                (unsigned long long)n_sel, n);
        return DBEEL_ERR_HIP;
    }
    if (stats) {
        stats->entries_in = n;
        stats->selected = n_sel;
        stats->entries = rd->mem.count;
        stats->data_bytes = rd->mem.data_len;
    }
    if (n_sel == 0) return DBEEL_OK; /* nothing selected: no put happened */
    hipLaunchKernelGGL(k_page_compact, grid, block, 0, s, n,
                       (const uint64_t*)b.pfx[1], (const uint32_t*)b.tie,
                       (const uint32_t*)b.tpos, b.pfx[0], b.arr[0]);

    /* 3-4. order and survivors, 5. encode + merge + swap */
    b.K = {d_data, nullptr, n, d_index};
    b.n = (uint32_t)n_sel;
    b.d_dts = tomb ? d_dts : nullptr;
    rc = batch_sort_flag(b, tomb, pg.data_len, s, rd->ev);
    if (rc) return rc;
    MemMerged mm;
    rc = mem_merge(who, rd, b, mm);
    if (rc) return rc;
    if (stats) {
        stats->h2d_ms = pg.on_device ? 0.0 : mm.ms[0];
        stats->order_ms = mm.ms[1];
        stats->merge_ms = mm.ms[2];
        stats->batch_entries = mm.batch_entries;
        stats->replaced = mm.replaced;
        stats->entries = mm.entries;
        stats->data_bytes = mm.data_bytes;
        stats->prefix_tied = b.prefix_tied;
    }
    return DBEEL_OK;
}

/* Host checks of put_entries, in the header's order. */
static int put_entries_check(const char* who, int mode,
                             const uint8_t* delete_ts) {
    if (mode != DBEEL_APPLY_PUT && mode != DBEEL_APPLY_DELETE) {
        set_err("%s: unknown mode %d", who, mode);
        return DBEEL_ERR_INVALID_ARG;
    }
    if (mode == DBEEL_APPLY_DELETE && !delete_ts) {
        set_err("%s: DELETE needs delete_ts", who);
        return DBEEL_ERR_INVALID_ARG;
    }
    return DBEEL_OK;
}

static int put_entries_count_check(const char* who, uint64_t n_mem,
                                   uint64_t n) {
    if (n >= (1ull << 31)) {
        set_err("%s: %llu entries, at most 2^31 - 1 per page", who,
                (unsigned long long)n);
        return DBEEL_ERR_INVALID_ARG;
    }
    if (n_mem + n >= (1ull << 31)) {
        set_err("%s: %llu memtable entries + %llu page entries, at most "
                "2^31 - 1 together (flush first)", who,
                (unsigned long long)n_mem, (unsigned long long)n);
        return DBEEL_ERR_INVALID_ARG;
    }
    return DBEEL_OK;
}

extern "C" int dbeel_gpu_reader_put_entries(
    dbeel_gpu_reader* rd, const uint8_t* data, uint64_t data_len,
    const uint8_t* index, uint64_t n_entries, const uint32_t* range_ids,
    const uint8_t* take, uint32_t n_take, int mode, const uint8_t* delete_ts,
    dbeel_put_entries_stats* stats) {
    g_err[0] = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    const char* who = "reader_put_entries";
    if (!rd) {
        set_err("%s: null reader", who);
        return DBEEL_ERR_INVALID_ARG;
    }
    if (n_entries && (!data || !index)) {
        set_err("%s: null data or index", who);
        return DBEEL_ERR_INVALID_ARG;
    }
    int rc = put_entries_check(who, mode, delete_ts);
    if (rc) return rc;
    if (range_ids && (!take || n_take == 0)) {
        set_err("%s: range_ids need a take mask with n_take > 0", who);
        return DBEEL_ERR_INVALID_ARG;
    }
    rc = put_entries_count_check(who, rd->mem.count, n_entries);
    if (rc) return rc;
    if (n_entries == 0) return DBEEL_OK;
    const PageIn pg = {data, data_len, index, n_entries, range_ids, false};
    return put_entries_impl(who, rd, pg, take, n_take, mode, delete_ts, stats);
}

extern "C" int dbeel_gpu_reader_memtable_info(const dbeel_gpu_reader* rd,
                                              dbeel_memtable_info* info) {
    g_err[0] = 0;
    if (info) memset(info, 0, sizeof *info);
    if (!rd || !info) {
        set_err("reader_memtable_info: null argument");
        return DBEEL_ERR_INVALID_ARG;
    }
    info->entries = rd->mem.count;
    info->data_bytes = rd->mem.data_len;
    info->reserved_bytes = rd->mem.reserved();
    info->puts = rd->mem.puts;
    return DBEEL_OK;
}

extern "C" int dbeel_gpu_reader_memtable_fetch(dbeel_gpu_reader* rd,
                                               dbeel_compact_result* out) {
    g_err[0] = 0;
    if (out) memset(out, 0, sizeof *out);
    if (!rd || !out) {
        set_err("reader_memtable_fetch: null argument");
        return DBEEL_ERR_INVALID_ARG;
    }
    const ReaderMemtable& M = rd->mem;
    if (!M.count) return DBEEL_OK;
    HIP_CHECK(hipSetDevice(rd->device));
    return batch_fetch(M.data(), M.data_len, M.index(), M.count, rd->stream,
                       out);
}

extern "C" void dbeel_gpu_reader_memtable_clear(dbeel_gpu_reader* rd) {
    if (rd) rd->mem.drop();
}

extern "C" int dbeel_gpu_reader_memtable_flush(dbeel_gpu_reader* rd,
                                               int build_bloom,
                                               dbeel_compact_result* out,
                                               uint8_t** bloom_bytes,
                                               uint64_t* bloom_len) {
    g_err[0] = 0;
    if (out) memset(out, 0, sizeof *out);
    if (bloom_bytes) *bloom_bytes = nullptr;
    if (bloom_len) *bloom_len = 0;
    if (!rd) {
        set_err("reader_memtable_flush: null reader");
        return DBEEL_ERR_INVALID_ARG;
    }
    if ((bloom_bytes == nullptr) != (bloom_len == nullptr)) {
        set_err("reader_memtable_flush: bloom_bytes and bloom_len go "
                "together");
        return DBEEL_ERR_INVALID_ARG;
    }
    ReaderMemtable& M = rd->mem;
    if (!M.count) return DBEEL_OK; /* lsm_tree.rs:850-852 */
    if (rd->tables.size() >= MAX_RUNS) {
        set_err("reader_memtable_flush: reader already holds %d runs",
                MAX_RUNS);
        return DBEEL_ERR_INVALID_ARG;
    }
    HIP_CHECK(hipSetDevice(rd->device));
    hipStream_t s = rd->stream;
    ReaderTable t;
    bool linked = false;
    ScopeGuard release([&] {
        if (linked) return;
        (void)hipStreamSynchronize(s);
        table_free(t);
        if (out) dbeel_gpu_result_free(out);
        if (bloom_bytes && *bloom_bytes) {
            free(*bloom_bytes);
            *bloom_bytes = nullptr;
            *bloom_len = 0;
        }
    });
    const uint64_t n_bits = build_bloom ? bloom_bits_for(M.count) : 0;
    HIP_CHECK(table_alloc(t, M.data_len, M.count, n_bits));
    HIP_CHECK(hipMemcpyAsync(t.d_run + 16, M.data(),
                             M.data_len + M.count * 16,
                             hipMemcpyDeviceToDevice, s));
    HIP_CHECK(table_adopt(t, n_bits, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    if (out) {
        int rc = batch_fetch(t.data(), t.data_len, t.index(), t.count, s, out);
        if (rc) return rc;
    }
    if (bloom_bytes && n_bits) {
        int rc = table_bloom_fetch(t, s, bloom_bytes, bloom_len);
        if (rc) return rc;
    }
    hipError_t e = reader_insert_table(rd, rd->tables.size(), t);
    HIP_CHECK(e); /* the guard above frees t */
    linked = true;
    M.drop();
    return DBEEL_OK;
}

extern "C" void dbeel_gpu_get_result_free(dbeel_get_result* r) {
    if (!r) return;
    free(r->hits);
    free(r->value_offsets);
    free(r->values);
    memset(r, 0, sizeof *r);
}

/* ---- The key batch of the read family (get, get_entries, get_merged):
 * one definition of what all three do before their paths part. ---- */

/* The two refusals of a key batch, under the caller's name. */
static int keys_check(const char* who, const uint64_t* key_offsets,
                      uint64_t n_keys) {
    if (n_keys >= (1ull << 32)) {
        set_err("%s: 2^32 or more keys in one batch", who);
        return DBEEL_ERR_INVALID_ARG;
    }
    for (uint64_t i = 0; i < n_keys; i++)
        if (key_offsets[i + 1] < key_offsets[i]) {
            set_err("%s: key_offsets not ascending at %llu", who,
                    (unsigned long long)i);
            return DBEEL_ERR_INVALID_ARG;
        }
    return DBEEL_OK;
}

/* d_batch layout: key offsets (n+1) | result offsets (n+1) | hits (n+1, the
 * last one a sentinel whose length is zero, so the scan's final element is
 * the total; which bytes say "zero length" is the caller's functor's
 * business, and so is writing them). */
struct KeyBatch {
    uint64_t* koff;
    uint64_t* roff;
    dbeel_lookup_hit* hits;
};

/* Reserves d_keys and d_batch for n keys and lays the batch out. */
static int keys_reserve(dbeel_gpu_reader* rd, const uint64_t* key_offsets,
                        uint64_t n, KeyBatch& kb) {
    const uint64_t kbytes = key_offsets[n];
    HIP_CHECK(reader_reserve((void**)&rd->d_keys, &rd->keys_cap,
                             kbytes ? kbytes : 1));
    HIP_CHECK(reader_reserve((void**)&rd->d_batch, &rd->batch_cap,
                             2 * (n + 1) * sizeof(uint64_t) +
                                 (n + 1) * sizeof(dbeel_lookup_hit)));
    kb.koff = (uint64_t*)rd->d_batch;
    kb.roff = kb.koff + (n + 1);
    kb.hits = (dbeel_lookup_hit*)(kb.roff + (n + 1));
    return DBEEL_OK;
}

/* Keys and offsets to the device, the search counters cleared. */
static int keys_upload(dbeel_gpu_reader* rd, const uint8_t* keys,
                       const uint64_t* key_offsets, uint64_t n,
                       const KeyBatch& kb) {
    hipStream_t s = rd->stream;
    const uint64_t kbytes = key_offsets[n];
    if (kbytes)
        HIP_CHECK(hipMemcpyAsync(rd->d_keys, keys, kbytes,
                                 hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(kb.koff, key_offsets,
                             (n + 1) * sizeof(uint64_t),
                             hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(rd->d_stats, 0, RS_N * sizeof(uint64_t), s));
    return DBEEL_OK;
}

/* Searches rd's tables (and its memtable, when it holds anything) for the n
 * keys on stream s: one hit record per key into `hits`, counters into rd's
 * d_stats. The keys may be another reader's upload (get_merged's sources). */
static void reader_search(const dbeel_gpu_reader* rd, hipStream_t s,
                          const uint8_t* d_keys, const uint64_t* d_koff,
                          uint64_t n, dbeel_lookup_hit* hits) {
    typedef void (*SearchFn)(RunsDesc, ReaderPfx, ReaderMem,
                             const ReaderBloom*, const uint8_t*,
                             const uint64_t*, uint64_t, dbeel_lookup_hit*,
                             unsigned long long*);
    SearchFn ks = k_reader_search<false>;
    if (rd->mem.count) ks = k_reader_search<true>;
    hipLaunchKernelGGL(ks, dim3(pick_grid(n, READER_BLOCK)),
                       dim3(READER_BLOCK), 0, s, rd->desc, rd->pfx,
                       rd->mem.view(), rd->d_blooms, d_keys, d_koff, n, hits,
                       rd->d_stats);
}

/* The search counters as get and get_entries report them. */
static void stats_counters(dbeel_get_stats* stats,
                           const unsigned long long* hstats) {
    stats->bloom_probes = hstats[RS_PROBES];
    stats->bloom_skips = hstats[RS_SKIPS];
    stats->searches = hstats[RS_SEARCHES];
    stats->hits = hstats[RS_HITS];
    stats->tombstones = hstats[RS_TOMBS];
}

extern "C" int dbeel_gpu_reader_get(dbeel_gpu_reader* rd,
                                    const uint8_t* keys,
                                    const uint64_t* key_offsets,
                                    uint64_t n_keys, dbeel_get_result* out,
                                    dbeel_get_stats* stats) {
    g_err[0] = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (!rd || !out || (n_keys && (!keys || !key_offsets))) {
        set_err("reader_get: null argument");
        return DBEEL_ERR_INVALID_ARG;
    }
    memset(out, 0, sizeof *out);
    if (int rc = keys_check("reader_get", key_offsets, n_keys)) return rc;
    const uint64_t n = n_keys;
    out->hits = (dbeel_lookup_hit*)malloc((n ? n : 1) * sizeof *out->hits);
    out->value_offsets = (uint64_t*)calloc(n + 1, sizeof(uint64_t));
    if (!out->hits || !out->value_offsets) {
        dbeel_gpu_get_result_free(out);
        set_err("host malloc failed");
        return DBEEL_ERR_OOM;
    }
    if (n == 0) {
        out->values = (uint8_t*)malloc(1);
        return DBEEL_OK;
    }

    const uint64_t off_bytes = (n + 1) * sizeof(uint64_t);
    size_t tmp_bytes = 0;
    uint64_t total = 0;
    unsigned long long hstats[RS_N] = {};
    float ms[6] = {};
    hipStream_t s = rd->stream;
    /* on failure nothing of this batch may still be in flight into freed
     * memory */
    ScopeGuard fail([&] {
        (void)hipStreamSynchronize(s);
        dbeel_gpu_get_result_free(out);
    });

    HIP_CHECK(hipSetDevice(rd->device));
    KeyBatch kb;
    if (int rc = keys_reserve(rd, key_offsets, n, kb)) return rc;
    uint64_t* d_voff = kb.roff;
    dbeel_lookup_hit* d_hits = kb.hits;
    HIP_CHECK(rocprim::exclusive_scan(
        nullptr, tmp_bytes,
        rocprim::make_transform_iterator(d_hits, HitValueLen{}), d_voff,
        (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), s));
    HIP_CHECK(reader_reserve(&rd->d_scantmp, &rd->scantmp_cap,
                             tmp_bytes ? tmp_bytes : 1));

    HIP_CHECK(hipEventRecord(rd->ev[0], s));
    if (int rc = keys_upload(rd, keys, key_offsets, n, kb)) return rc;
    /* the sentinel: zeroed, value_len 0 */
    HIP_CHECK(hipMemsetAsync(d_hits + n, 0, sizeof(dbeel_lookup_hit), s));
    HIP_CHECK(hipEventRecord(rd->ev[1], s));
    reader_search(rd, s, rd->d_keys, kb.koff, n, d_hits);
    HIP_CHECK(hipEventRecord(rd->ev[2], s));
    HIP_CHECK(rocprim::exclusive_scan(
        rd->d_scantmp, tmp_bytes,
        rocprim::make_transform_iterator(d_hits, HitValueLen{}), d_voff,
        (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), s));
    HIP_CHECK(hipEventRecord(rd->ev[3], s));
    HIP_CHECK(hipMemcpyAsync(&total, d_voff + n, 8, hipMemcpyDeviceToHost,
                             s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    out->values = (uint8_t*)malloc(total ? total : 1);
    if (!out->values) {
        set_err("host malloc of %llu value bytes failed",
                (unsigned long long)total);
        return DBEEL_ERR_OOM;
    }
    if (total)
        HIP_CHECK(reader_reserve((void**)&rd->d_values, &rd->values_cap,
                                 total));
    HIP_CHECK(hipEventRecord(rd->ev[4], s));
    if (total)
        hipLaunchKernelGGL(k_reader_gather, dim3(pick_grid(n * 64, 256)),
                           dim3(256), 0, s, rd->desc, rd->mem.view().data,
                           d_hits, d_voff, n, rd->d_values);
    HIP_CHECK(hipEventRecord(rd->ev[5], s));
    HIP_CHECK(hipMemcpyAsync(out->hits, d_hits, n * sizeof *out->hits,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(out->value_offsets, d_voff, off_bytes,
                             hipMemcpyDeviceToHost, s));
    if (total)
        HIP_CHECK(hipMemcpyAsync(out->values, rd->d_values, total,
                                 hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(hstats, rd->d_stats, sizeof hstats,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipEventRecord(rd->ev[6], s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    for (int i = 0; i < 6; i++)
        HIP_CHECK(hipEventElapsedTime(&ms[i], rd->ev[i], rd->ev[i + 1]));
    out->values_len = total;
    out->n_keys = n;
    if (stats) {
        stats->h2d_ms = ms[0];
        stats->search_ms = ms[1];
        stats->gather_ms = ms[2] + ms[4]; /* scan + gather kernel; the
                                             host gap between them (ms[3],
                                             sizing the output) is not
                                             device work */
        stats->d2h_ms = ms[5];
        stats_counters(stats, hstats);
    }
    fail.dismiss();
    return DBEEL_OK;
}

/* ------------------------------------------------------------------ */
/* get_entries: LSMTree::get_entry's answer (lsm_tree.rs:674-723),    */
/* EntryValue { data, timestamp }, into caller buffers                */
/*                                                                    */
/* A stored entry ends in data_len:u64 | data | timestamp:i128, which */
/* is the bincode form of EntryValue: the record of a hit is those    */
/* 24 + value_len bytes, copied verbatim. The search is reader_get's  */
/* kernel, launched the same way; only what follows it differs.       */
/* ------------------------------------------------------------------ */

/* Record size of a hit. A found tombstone is a 24-B record, so the zeroed
 * sentinel reader_get appends (run 0, value_len 0) would count here: this
 * path's sentinel is run = -1. */
struct HitRecordLen {
    __device__ uint64_t operator()(const dbeel_lookup_hit& h) const {
        return h.run < 0 ? 0 : h.value_len + 24;
    }
};

/* One wave per delivered query copies data_len | data | timestamp, the
 * entry's bytes from value_offset - 8 to its end, reading exactly the record
 * and writing exactly the record. Tombstones are copied like any hit. The
 * bounds are those validated at open (off + full_size <= data_len). */
__global__ void k_reader_gather_entries(RunsDesc R, const uint8_t* mem_data,
                                        const dbeel_lookup_hit* hits,
                                        const uint64_t* rec_off,
                                        uint64_t n_done, uint8_t* records) {
    uint32_t lane = threadIdx.x & 63;
    uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t q = wave; q < n_done; q += n_waves) {
        const dbeel_lookup_hit h = hits[q];
        if (h.run < 0) continue;
        /* run == n_runs names the memtable; with 64 tables that index lies
         * past R's arrays, so it is resolved before any of them is read */
        const uint8_t* src = h.run >= R.n_runs ? mem_data : R.data[h.run];
        wave_copy_bytes(records + rec_off[q], src + h.value_offset - 8,
                        h.value_len + 24, lane);
    }
}

extern "C" int dbeel_gpu_reader_get_entries(
    dbeel_gpu_reader* rd, const uint8_t* keys, const uint64_t* key_offsets,
    uint64_t n_keys, const dbeel_get_buffers* buf, dbeel_get_page* page,
    dbeel_get_stats* stats) {
    g_err[0] = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    if (page) memset(page, 0, sizeof *page);
    if (!rd || !buf || !page) {
        set_err("reader_get_entries: null reader, buf or page");
        return DBEEL_ERR_INVALID_ARG;
    }
    if (n_keys &&
        (!keys || !key_offsets || !buf->hits || !buf->record_offsets)) {
        set_err("reader_get_entries: null keys, key_offsets, hits or "
                "record_offsets");
        return DBEEL_ERR_INVALID_ARG;
    }
    if (!buf->records && buf->records_cap) {
        set_err("reader_get_entries: null records with records_cap %llu",
                (unsigned long long)buf->records_cap);
        return DBEEL_ERR_INVALID_ARG;
    }
    if (int rc = keys_check("reader_get_entries", key_offsets, n_keys))
        return rc;
    const uint64_t n = n_keys;
    if (n == 0) {
        if (buf->record_offsets) buf->record_offsets[0] = 0;
        return DBEEL_OK;
    }

    const uint64_t off_bytes = (n + 1) * sizeof(uint64_t);
    size_t tmp_bytes = 0;
    unsigned long long hstats[RS_N] = {};
    float ms[6] = {};
    hipStream_t s = rd->stream;
    /* on failure nothing of this batch may still be in flight into the
     * caller's buffers */
    ScopeGuard fail([&] { (void)hipStreamSynchronize(s); });

    HIP_CHECK(hipSetDevice(rd->device));
    KeyBatch kb;
    if (int rc = keys_reserve(rd, key_offsets, n, kb)) return rc;
    uint64_t* d_roff = kb.roff;
    dbeel_lookup_hit* d_hits = kb.hits;
    HIP_CHECK(rocprim::exclusive_scan(
        nullptr, tmp_bytes,
        rocprim::make_transform_iterator(d_hits, HitRecordLen{}), d_roff,
        (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), s));
    HIP_CHECK(reader_reserve(&rd->d_scantmp, &rd->scantmp_cap,
                             tmp_bytes ? tmp_bytes : 1));

    HIP_CHECK(hipEventRecord(rd->ev[0], s));
    if (int rc = keys_upload(rd, keys, key_offsets, n, kb)) return rc;
    /* the sentinel: all-ones bytes, run = -1 */
    HIP_CHECK(hipMemsetAsync(d_hits + n, 0xFF, sizeof(dbeel_lookup_hit), s));
    HIP_CHECK(hipEventRecord(rd->ev[1], s));
    reader_search(rd, s, rd->d_keys, kb.koff, n, d_hits);
    HIP_CHECK(hipEventRecord(rd->ev[2], s));
    HIP_CHECK(rocprim::exclusive_scan(
        rd->d_scantmp, tmp_bytes,
        rocprim::make_transform_iterator(d_hits, HitRecordLen{}), d_roff,
        (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), s));
    HIP_CHECK(hipEventRecord(rd->ev[3], s));
    /* hits and offsets go out complete whatever the cap; the offsets are
     * what the host sizes the page from */
    HIP_CHECK(hipMemcpyAsync(buf->record_offsets, d_roff, off_bytes,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(buf->hits, d_hits, n * sizeof *buf->hits,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(hstats, rd->d_stats, sizeof hstats,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipEventRecord(rd->ev[4], s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    for (int i = 0; i < 4; i++)
        HIP_CHECK(hipEventElapsedTime(&ms[i], rd->ev[i], rd->ev[i + 1]));

    /* n_done = the largest d with record_offsets[d] <= records_cap, by
     * bisection over the ascending offsets (offsets[0] = 0 always fits) */
    const uint64_t* off = buf->record_offsets;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= buf->records_cap)
            lo = mid;
        else
            hi = mid - 1;
    }
    const uint64_t n_done = lo, len = off[n_done];
    page->n_done = n_done;
    page->records_len = len;
    page->records_total = off[n];
    /* record n_done did not fit, so it is not empty */
    page->needed = n_done < n ? off[n_done + 1] - off[n_done] : 0;

    if (len) {
        HIP_CHECK(reader_reserve((void**)&rd->d_values, &rd->values_cap,
                                 len));
        HIP_CHECK(hipEventRecord(rd->ev[4], s));
        hipLaunchKernelGGL(k_reader_gather_entries,
                           dim3(pick_grid(n_done * 64, 256)), dim3(256), 0, s,
                           rd->desc, rd->mem.view().data, d_hits, d_roff,
                           n_done, rd->d_values);
        HIP_CHECK(hipEventRecord(rd->ev[5], s));
        HIP_CHECK(hipMemcpyAsync(buf->records, rd->d_values, len,
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipEventRecord(rd->ev[6], s));
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventElapsedTime(&ms[4], rd->ev[4], rd->ev[5]));
        HIP_CHECK(hipEventElapsedTime(&ms[5], rd->ev[5], rd->ev[6]));
    }
    if (stats) {
        stats->h2d_ms = ms[0];
        stats->search_ms = ms[1];
        stats->gather_ms = ms[2] + ms[4]; /* offset scan + record gather */
        stats->d2h_ms = ms[3] + ms[5];    /* every copy to the caller    */
        stats_counters(stats, hstats);
    }
    fail.dismiss();
    if (n_done == 0) { /* n > 0: record 0 alone is over the cap */
        set_err("reader_get_entries: record 0 needs %llu bytes, "
                "records_cap is %llu", (unsigned long long)page->needed,
                (unsigned long long)buf->records_cap);
        return DBEEL_ERR_ITEM_TOO_LARGE;
    }
    return DBEEL_OK;
}

/* ------------------------------------------------------------------ */
/* get_merged: the replicated read (tasks/db_server.rs:338-363)       */
/*                                                                    */
/* The reference collects the replicas' Option<EntryValue> answers,   */
/* pushes the local one last, takes max_by_key(timestamp) and only    */
/* then tests for a tombstone. Here every candidate — another reader  */
/* on this device, or a replica's get_entries answer uploaded from    */
/* the host — is reduced to one {address, length} per query, the      */
/* newest is picked per query on the device, and only the winners'    */
/* records are gathered and leave the device.                         */
/*                                                                    */
/*   k_reader_search : per reader candidate, launched as get_entries  */
/*                     launches it (a source reader on its own stream */
/*                     into its own scratch).                         */
/*   k_merge_stage   : one launch per candidate: hit records or       */
/*                     answer offsets -> cand[candidate][query];      */
/*                     uploaded records are validated here.           */
/*   k_merge_pick    : thread per query: newest timestamp, ties to    */
/*                     the later candidate, stale mask, counters.     */
/*   rocPRIM scan    : winner lengths -> exclusive record offsets.    */
/*   k_merge_page    : the paging rule on the device, so the offsets  */
/*                     reach the caller only once the call is known   */
/*                     to succeed.                                    */
/*   k_merge_gather  : wave per delivered query, from the winner's    */
/*                     absolute address.                              */
/* ------------------------------------------------------------------ */

/* One candidate's answer to one query; len == 0 = absent. */
struct MergeCand {
    const uint8_t* rec;
    uint64_t len;
};
static_assert(sizeof(MergeCand) == 16, "cand entries are 16 B");

struct CandLen {
    __device__ uint64_t operator()(const MergeCand& c) const { return c.len; }
};

enum { MS_WINNERS, MS_TOMBS, MS_LOCAL, MS_N };
#define MERGE_NO_ERR 0xFFFFFFFFFFFFFFFFull

/* What k_merge_page leaves for the host's one mid-call read: the counters,
 * the first corrupt answer as source << 32 | query (MERGE_NO_ERR = none;
 * atomicMin keeps the lowest) and the page. */
struct MergeTotals {
    unsigned long long stats[MS_N];
    unsigned long long err;
    dbeel_get_page page;
};

/* hits != NULL: a reader candidate, its hit records resolved through its own
 * descriptor and memtable (k_reader_gather_entries' addressing). Otherwise an
 * uploaded answer: rec_off / rec are its n + 1 offsets and record bytes on
 * the device. The host has checked that the offsets ascend from 0, so every
 * range lies inside the upload; a record that cannot be an EntryValue
 * (shorter than 24 bytes, or a data_len that is not its size - 24) is
 * reported and staged as absent. */
__global__ void k_merge_stage(RunsDesc R, const uint8_t* mem_data,
                              const dbeel_lookup_hit* hits,
                              const uint64_t* rec_off, const uint8_t* rec,
                              uint64_t n, uint32_t source, MergeCand* out,
                              unsigned long long* err) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n;
         q += stride) {
        MergeCand c = {nullptr, 0};
        if (hits) {
            const dbeel_lookup_hit h = hits[q];
            if (h.run >= 0) {
                const uint8_t* src =
                    h.run >= R.n_runs ? mem_data : R.data[h.run];
                c.rec = src + h.value_offset - 8;
                c.len = h.value_len + 24;
            }
        } else {
            const uint64_t o = rec_off[q], len = rec_off[q + 1] - o;
            if (len) {
                if (len < 24 || ld_u64(rec + o) != len - 24) {
                    atomicMin(err, ((unsigned long long)source << 32) | q);
                } else {
                    c.rec = rec + o;
                    c.len = len;
                }
            }
        }
        out[q] = c;
    }
}

/* cand is [n_cand][n]: a wave reads 64 consecutive entries of one candidate.
 * The timestamp is the record's last 16 bytes, i128 little-endian, loaded as
 * bytes (records are byte-aligned at best) and compared as a signed high
 * half, then an unsigned low half. `tied` holds the candidates equal to the
 * best so far, so one pass yields the stale mask: a newer candidate makes
 * all of them stale, an older one is stale itself, and the winner is the
 * highest tied index (max_by_key returns the last maximum). */
__global__ __launch_bounds__(256) void k_merge_pick(
    const MergeCand* cand, uint32_t n_cand, uint64_t n, dbeel_merge_hit* hits,
    MergeCand* win, unsigned long long* stats) {
    __shared__ unsigned long long s_stats[MS_N];
    if (threadIdx.x < MS_N) s_stats[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long cnt[MS_N] = {};
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n;
         q += stride) {
        MergeCand best = {nullptr, 0};
        int64_t bhi = 0;
        uint64_t blo = 0;
        uint32_t tied = 0, stale = 0, absent = 0;
        for (uint32_t c = 0; c < n_cand; c++) {
            const MergeCand m = cand[(uint64_t)c * n + q];
            if (!m.len) {
                absent |= 1u << c;
                continue;
            }
            const uint64_t lo = ld_u64(m.rec + m.len - 16);
            const int64_t hi = (int64_t)ld_u64(m.rec + m.len - 8);
            if (tied && (hi < bhi || (hi == bhi && lo < blo))) {
                stale |= 1u << c;
                continue;
            }
            if (tied && hi == bhi && lo == blo) {
                tied |= 1u << c;
            } else {
                stale |= tied;
                tied = 1u << c;
                bhi = hi;
                blo = lo;
            }
            best = m;
        }
        dbeel_merge_hit h;
        h.source = tied ? 31 - __clz((int)tied) : -1;
        h.is_tombstone = best.len == 24 ? 1 : 0;
        h.value_len = best.len ? best.len - 24 : 0;
        h.stale_mask = tied ? (uint64_t)(stale | absent) : 0;
        hits[q] = h;
        win[q] = best;
        if (tied) {
            cnt[MS_WINNERS]++;
            if (best.len == 24) cnt[MS_TOMBS]++;
            if (h.source == (int32_t)n_cand - 1) cnt[MS_LOCAL]++;
        }
    }
    #pragma unroll
    for (int s = 0; s < MS_N; s++)
        if (cnt[s]) atomicAdd(&s_stats[s], cnt[s]);
    __syncthreads();
    if (threadIdx.x < MS_N && s_stats[threadIdx.x])
        atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
}

/* get_entries' paging rule on the n + 1 ascending offsets: n_done is the
 * largest d with off[d] <= cap, and exactly one d in [0, n] has
 * off[d] <= cap with d == n or off[d + 1] > cap (off[0] = 0 always fits). */
__global__ void k_merge_page(const uint64_t* off, uint64_t n, uint64_t cap,
                             dbeel_get_page* page) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; d <= n;
         d += stride) {
        if (off[d] > cap || (d < n && off[d + 1] <= cap)) continue;
        page->n_done = d;
        page->records_len = off[d];
        page->records_total = off[n];
        page->needed = d < n ? off[d + 1] - off[d] : 0;
    }
}

/* One wave per delivered query copies the winner's record verbatim, reading
 * exactly the record and writing exactly the record. */
__global__ void k_merge_gather(const MergeCand* win, const uint64_t* rec_off,
                               uint64_t n_done, uint8_t* records) {
    uint32_t lane = threadIdx.x & 63;
    uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t q = wave; q < n_done; q += n_waves) {
        const MergeCand w = win[q];
        if (!w.len) continue;
        wave_copy_bytes(records + rec_off[q], w.rec, w.len, lane);
    }
}

static inline uint64_t round8(uint64_t x) { return (x + 7) & ~7ull; }

extern "C" int dbeel_gpu_reader_get_merged(
    dbeel_gpu_reader* rd, const uint8_t* keys, const uint64_t* key_offsets,
    uint64_t n_keys, const dbeel_merge_source* sources, size_t n_sources,
    const dbeel_merge_buffers* buf, dbeel_get_page* page,
    dbeel_merge_stats* stats) {
    g_err[0] = 0;
    const char* who = "reader_get_merged";
    if (stats) memset(stats, 0, sizeof *stats);
    if (page) memset(page, 0, sizeof *page);
    if (!rd || !buf || !page) {
        set_err("%s: null reader, buf or page", who);
        return DBEEL_ERR_INVALID_ARG;
    }
    if (n_keys &&
        (!keys || !key_offsets || !buf->hits || !buf->record_offsets)) {
        set_err("%s: null keys, key_offsets, hits or record_offsets", who);
        return DBEEL_ERR_INVALID_ARG;
    }
    if (!buf->records && buf->records_cap) {
        set_err("%s: null records with records_cap %llu", who,
                (unsigned long long)buf->records_cap);
        return DBEEL_ERR_INVALID_ARG;
    }
    if (int rc = keys_check(who, key_offsets, n_keys)) return rc;
    if (n_sources > DBEEL_MERGE_MAX_SOURCES) {
        set_err("%s: %zu sources, at most %d", who, n_sources,
                DBEEL_MERGE_MAX_SOURCES);
        return DBEEL_ERR_INVALID_ARG;
    }
    if (n_sources && !sources) {
        set_err("%s: null sources with n_sources %zu", who, n_sources);
        return DBEEL_ERR_INVALID_ARG;
    }
    for (size_t i = 0; i < n_sources; i++)
        if (sources[i].kind != DBEEL_MERGE_ANSWERS &&
            sources[i].kind != DBEEL_MERGE_READER) {
            set_err("%s: source %zu has unknown kind %d", who, i,
                    sources[i].kind);
            return DBEEL_ERR_INVALID_ARG;
        }
    for (size_t i = 0; i < n_sources; i++) {
        if (sources[i].kind != DBEEL_MERGE_READER) continue;
        const dbeel_gpu_reader* sr = sources[i].reader;
        if (!sr) {
            set_err("%s: source %zu has no reader", who, i);
            return DBEEL_ERR_INVALID_ARG;
        }
        if (sr == rd) {
            set_err("%s: source %zu is the local reader itself", who, i);
            return DBEEL_ERR_INVALID_ARG;
        }
        if (sr->device != rd->device) {
            set_err("%s: source %zu's reader is on device %d, the local one "
                    "on device %d", who, i, sr->device, rd->device);
            return DBEEL_ERR_INVALID_ARG;
        }
    }
    for (size_t i = 0; i < n_sources; i++) {
        if (sources[i].kind != DBEEL_MERGE_ANSWERS) continue;
        if (!sources[i].record_offsets) {
            set_err("%s: source %zu has null record_offsets", who, i);
            return DBEEL_ERR_INVALID_ARG;
        }
        if (!sources[i].records && sources[i].record_offsets[n_keys]) {
            set_err("%s: source %zu has null records with %llu record bytes",
                    who, i,
                    (unsigned long long)sources[i].record_offsets[n_keys]);
            return DBEEL_ERR_INVALID_ARG;
        }
    }
    for (size_t i = 0; i < n_sources; i++) {
        if (sources[i].kind != DBEEL_MERGE_ANSWERS) continue;
        const uint64_t* o = sources[i].record_offsets;
        if (o[0] != 0) {
            set_err("%s: source %zu's record_offsets start at %llu, not 0",
                    who, i, (unsigned long long)o[0]);
            return DBEEL_ERR_INVALID_ARG;
        }
        for (uint64_t q = 0; q < n_keys; q++)
            if (o[q + 1] < o[q]) {
                set_err("%s: source %zu's record_offsets not ascending at "
                        "%llu", who, i, (unsigned long long)q);
                return DBEEL_ERR_INVALID_ARG;
            }
    }
    const uint64_t n = n_keys;
    if (n == 0) {
        if (buf->record_offsets) buf->record_offsets[0] = 0;
        return DBEEL_OK;
    }

    const uint32_t n_cand = (uint32_t)n_sources + 1;
    const uint64_t off_bytes = (n + 1) * sizeof(uint64_t);
    /* the uploaded answers, each as offsets | records, 8-B aligned */
    uint64_t ans_bytes = 0;
    for (size_t i = 0; i < n_sources; i++)
        if (sources[i].kind == DBEEL_MERGE_ANSWERS)
            ans_bytes += off_bytes + round8(sources[i].record_offsets[n]);
    /* d_merge layout: cand (n_cand * n) | winners (n + 1, the last one absent
     * so the scan's final element is the total) | record offsets (n + 1) |
     * merge hits (n) | totals */
    const uint64_t cand_bytes = (uint64_t)n_cand * n * sizeof(MergeCand);
    const uint64_t merge_bytes = cand_bytes + (n + 1) * sizeof(MergeCand) +
                                 off_bytes + n * sizeof(dbeel_merge_hit) +
                                 sizeof(MergeTotals);
    size_t tmp_bytes = 0;
    MergeTotals tot;
    float ms[7] = {};
    double search_ms = 0;
    hipStream_t s = rd->stream;
    /* on failure nothing of this batch may still be in flight into the
     * caller's buffers or out of a source's scratch */
    ScopeGuard fail([&] {
        (void)hipStreamSynchronize(s);
        for (size_t i = 0; i < n_sources; i++)
            if (sources[i].kind == DBEEL_MERGE_READER)
                (void)hipStreamSynchronize(sources[i].reader->stream);
    });

    HIP_CHECK(hipSetDevice(rd->device));
    /* the key batch's result-offset slot and sentinel hit are unused here:
     * the offsets scanned are the winners', in d_merge. kb's pointers stay
     * good through the sources' reservations below only because no source
     * is rd itself (refused above): those grow other readers' d_batch. */
    KeyBatch kb;
    if (int rc = keys_reserve(rd, key_offsets, n, kb)) return rc;
    HIP_CHECK(reader_reserve((void**)&rd->d_merge, &rd->merge_cap,
                             merge_bytes));
    HIP_CHECK(reader_reserve((void**)&rd->d_answers, &rd->answers_cap,
                             ans_bytes ? ans_bytes : 1));
    for (size_t i = 0; i < n_sources; i++)
        if (sources[i].kind == DBEEL_MERGE_READER) {
            dbeel_gpu_reader* sr = sources[i].reader;
            HIP_CHECK(reader_reserve((void**)&sr->d_batch, &sr->batch_cap,
                                     n * sizeof(dbeel_lookup_hit)));
        }
    MergeCand* d_cand = (MergeCand*)rd->d_merge;
    MergeCand* d_win = d_cand + (uint64_t)n_cand * n;
    uint64_t* d_roff = (uint64_t*)(d_win + (n + 1));
    dbeel_merge_hit* d_mhits = (dbeel_merge_hit*)(d_roff + (n + 1));
    MergeTotals* d_tot = (MergeTotals*)(d_mhits + n);
    HIP_CHECK(rocprim::exclusive_scan(
        nullptr, tmp_bytes,
        rocprim::make_transform_iterator(d_win, CandLen{}), d_roff,
        (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), s));
    HIP_CHECK(reader_reserve(&rd->d_scantmp, &rd->scantmp_cap,
                             tmp_bytes ? tmp_bytes : 1));

    HIP_CHECK(hipEventRecord(rd->ev[0], s));
    if (int rc = keys_upload(rd, keys, key_offsets, n, kb)) return rc;
    uint64_t ans_at = 0;
    for (size_t i = 0; i < n_sources; i++) {
        if (sources[i].kind != DBEEL_MERGE_ANSWERS) continue;
        const uint64_t rb = sources[i].record_offsets[n];
        HIP_CHECK(hipMemcpyAsync(rd->d_answers + ans_at,
                                 sources[i].record_offsets, off_bytes,
                                 hipMemcpyHostToDevice, s));
        if (rb)
            HIP_CHECK(hipMemcpyAsync(rd->d_answers + ans_at + off_bytes,
                                     sources[i].records, rb,
                                     hipMemcpyHostToDevice, s));
        ans_at += off_bytes + round8(rb);
    }
    HIP_CHECK(hipMemsetAsync(d_tot, 0, sizeof *d_tot, s));
    HIP_CHECK(hipMemsetAsync(&d_tot->err, 0xFF, sizeof d_tot->err, s));
    HIP_CHECK(hipMemsetAsync(d_win + n, 0, sizeof(MergeCand), s));
    HIP_CHECK(hipEventRecord(rd->ev[1], s));

    /* every reader candidate is searched as get_entries searches it; a
     * source on its own stream, once the keys are up, into its own scratch */
    for (size_t i = 0; i < n_sources; i++) {
        if (sources[i].kind != DBEEL_MERGE_READER) continue;
        dbeel_gpu_reader* sr = sources[i].reader;
        HIP_CHECK(hipStreamWaitEvent(sr->stream, rd->ev[1], 0));
        HIP_CHECK(hipMemsetAsync(sr->d_stats, 0, RS_N * sizeof(uint64_t),
                                 sr->stream));
        HIP_CHECK(hipEventRecord(sr->ev[0], sr->stream));
        reader_search(sr, sr->stream, rd->d_keys, kb.koff, n,
                      (dbeel_lookup_hit*)sr->d_batch);
        HIP_CHECK(hipEventRecord(sr->ev[1], sr->stream));
    }
    reader_search(rd, s, rd->d_keys, kb.koff, n, kb.hits);
    HIP_CHECK(hipEventRecord(rd->ev[2], s));
    /* a source's hit records are read on the local stream: its own stream
     * is drained first */
    for (size_t i = 0; i < n_sources; i++) {
        if (sources[i].kind != DBEEL_MERGE_READER) continue;
        dbeel_gpu_reader* sr = sources[i].reader;
        HIP_CHECK(hipStreamSynchronize(sr->stream));
        float t = 0;
        HIP_CHECK(hipEventElapsedTime(&t, sr->ev[0], sr->ev[1]));
        search_ms += t;
    }
    HIP_CHECK(hipGetLastError());

    HIP_CHECK(hipEventRecord(rd->ev[6], s));
    const dim3 grid_n(pick_grid(n, 256)), block(256);
    ans_at = 0;
    for (uint32_t c = 0; c < n_cand; c++) {
        MergeCand* out = d_cand + (uint64_t)c * n;
        if (c == n_sources) {
            hipLaunchKernelGGL(k_merge_stage, grid_n, block, 0, s, rd->desc,
                               rd->mem.view().data, kb.hits, nullptr, nullptr,
                               n, c, out, &d_tot->err);
        } else if (sources[c].kind == DBEEL_MERGE_READER) {
            const dbeel_gpu_reader* sr = sources[c].reader;
            hipLaunchKernelGGL(k_merge_stage, grid_n, block, 0, s, sr->desc,
                               sr->mem.view().data,
                               (const dbeel_lookup_hit*)sr->d_batch, nullptr,
                               nullptr, n, c, out, &d_tot->err);
        } else {
            const uint8_t* a = rd->d_answers + ans_at;
            hipLaunchKernelGGL(k_merge_stage, grid_n, block, 0, s, RunsDesc{},
                               nullptr, nullptr, (const uint64_t*)a,
                               a + off_bytes, n, c, out, &d_tot->err);
            ans_at += off_bytes + round8(sources[c].record_offsets[n]);
        }
    }
    hipLaunchKernelGGL(k_merge_pick, grid_n, block, 0, s, d_cand, n_cand, n,
                       d_mhits, d_win, d_tot->stats);
    HIP_CHECK(hipEventRecord(rd->ev[3], s));
    HIP_CHECK(rocprim::exclusive_scan(
        rd->d_scantmp, tmp_bytes,
        rocprim::make_transform_iterator(d_win, CandLen{}), d_roff,
        (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), s));
    hipLaunchKernelGGL(k_merge_page, dim3(pick_grid(n + 1, 256)), block, 0, s,
                       d_roff, n, buf->records_cap, &d_tot->page);
    HIP_CHECK(hipEventRecord(rd->ev[4], s));
    /* the one mid-call read: counters, error word and page. The caller's
     * buffers are written only after the error word is known to be clear. */
    HIP_CHECK(hipMemcpyAsync(&tot, d_tot, sizeof tot, hipMemcpyDeviceToHost,
                             s));
    HIP_CHECK(hipEventRecord(rd->ev[5], s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventElapsedTime(&ms[0], rd->ev[0], rd->ev[1]));
    HIP_CHECK(hipEventElapsedTime(&ms[1], rd->ev[1], rd->ev[2]));
    HIP_CHECK(hipEventElapsedTime(&ms[2], rd->ev[6], rd->ev[3]));
    HIP_CHECK(hipEventElapsedTime(&ms[3], rd->ev[3], rd->ev[4]));
    HIP_CHECK(hipEventElapsedTime(&ms[4], rd->ev[4], rd->ev[5]));
    if (tot.err != MERGE_NO_ERR) {
        fail.dismiss(); /* every stream is idle */
        set_err("%s: source %llu's answer to query %llu is not an "
                "EntryValue record (shorter than 24 bytes, or its data_len "
                "is not its size - 24)", who, tot.err >> 32,
                tot.err & 0xFFFFFFFFull);
        return DBEEL_ERR_CORRUPT;
    }
    *page = tot.page;
    const uint64_t n_done = page->n_done, len = page->records_len;

    if (len)
        HIP_CHECK(reader_reserve((void**)&rd->d_values, &rd->values_cap,
                                 len));
    HIP_CHECK(hipEventRecord(rd->ev[4], s));
    if (len)
        hipLaunchKernelGGL(k_merge_gather,
                           dim3(pick_grid(n_done * 64, 256)), block, 0, s,
                           d_win, d_roff, n_done, rd->d_values);
    HIP_CHECK(hipEventRecord(rd->ev[5], s));
    /* hits and offsets go out complete whatever the cap */
    HIP_CHECK(hipMemcpyAsync(buf->record_offsets, d_roff, off_bytes,
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(buf->hits, d_mhits, n * sizeof *buf->hits,
                             hipMemcpyDeviceToHost, s));
    if (len)
        HIP_CHECK(hipMemcpyAsync(buf->records, rd->d_values, len,
                                 hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipEventRecord(rd->ev[6], s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventElapsedTime(&ms[5], rd->ev[4], rd->ev[5]));
    HIP_CHECK(hipEventElapsedTime(&ms[6], rd->ev[5], rd->ev[6]));
    if (stats) {
        stats->h2d_ms = ms[0];
        stats->search_ms = ms[1] + search_ms; /* the search kernels' own
                                                 times; sources overlap the
                                                 local one                */
        stats->pick_ms = ms[2];               /* stage launches + pick    */
        stats->gather_ms = ms[3] + ms[5];     /* scan, page, gather       */
        stats->d2h_ms = ms[4] + ms[6];        /* every copy to the host   */
        stats->winners = tot.stats[MS_WINNERS];
        stats->tombstones = tot.stats[MS_TOMBS];
        stats->from_local = tot.stats[MS_LOCAL];
    }
    fail.dismiss();
    if (n_done == 0) { /* n > 0: record 0 alone is over the cap */
        set_err("%s: record 0 needs %llu bytes, records_cap is %llu", who,
                (unsigned long long)page->needed,
                (unsigned long long)buf->records_cap);
        return DBEEL_ERR_ITEM_TOO_LARGE;
    }
    return DBEEL_OK;
}

extern "C" int dbeel_gpu_reader_compact_fetch(
    dbeel_gpu_reader* rd, uint8_t* data, uint64_t data_cap, uint8_t* index,
    uint64_t index_cap, uint64_t* data_len, uint64_t* index_len,
    double* d2h_ms) {
    g_err[0] = 0;
    if (data_len) *data_len = 0;
    if (index_len) *index_len = 0;
    if (d2h_ms) *d2h_ms = 0;
    if (!rd || !data || !index || !data_len || !index_len) {
        set_err("reader_compact_fetch: null argument");
        return DBEEL_ERR_INVALID_ARG;
    }
    if (!rd->has_pending) {
        set_err("reader_compact_fetch: no compaction pending");
        return DBEEL_ERR_INVALID_ARG;
    }
    const ReaderTable& t = rd->pending;
    const uint64_t dl = t.data_len, il = t.count * 16;
    *data_len = dl;
    *index_len = il;
    if (dl > data_cap || il > index_cap) {
        set_err("reader_compact_fetch: output needs %llu data and %llu index "
                "bytes, caps are %llu and %llu", (unsigned long long)dl,
                (unsigned long long)il, (unsigned long long)data_cap,
                (unsigned long long)index_cap);
        return DBEEL_ERR_ITEM_TOO_LARGE;
    }
    hipStream_t s = rd->stream;
    ScopeGuard fail([&] { (void)hipStreamSynchronize(s); });
    HIP_CHECK(hipSetDevice(rd->device));
    HIP_CHECK(hipEventRecord(rd->ev[0], s));
    if (dl)
        HIP_CHECK(hipMemcpyAsync(data, t.data(), dl, hipMemcpyDeviceToHost,
                                 s));
    if (il)
        HIP_CHECK(hipMemcpyAsync(index, t.index(), il, hipMemcpyDeviceToHost,
                                 s));
    HIP_CHECK(hipEventRecord(rd->ev[1], s));
    HIP_CHECK(hipStreamSynchronize(s));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, rd->ev[0], rd->ev[1]));
    if (d2h_ms) *d2h_ms = ms;
    fail.dismiss();
    return DBEEL_OK;
}

/* ------------------------------------------------------------------ */
/* Migration / iteration scan (AsyncIter analogue)                    */
/*                                                                    */
/* See include/dbeel_gpu.h. The yield order is the reference's:       */
/* sstables ascending, entries in index order within each             */
/* (lsm_tree.rs:210-276) — which is exactly the global entry order g, */
/* so the existing survivor-scan/emit/copy machinery packs the        */
/* filtered entries verbatim. No dedup, no tombstone filter.          */
/* ------------------------------------------------------------------ */

/* MurmurHash3 x86_32 — restatement of the murmur3 crate v0.5.2's      */
/* murmur3_32 (the reference's hash_bytes, shards.rs:96-101, seed 0   */
/* everywhere). Public algorithm (Appleby); pinned by the published   */
/* test vectors in tests/test_scan_host.py.                           */
__device__ __host__ __forceinline__ uint32_t rotl32(uint32_t x, int r) {
    return (x << r) | (x >> (32 - r));
}
__device__ __host__ inline uint32_t murmur3_32(const uint8_t* key,
                                               uint64_t len,
                                               uint32_t seed) {
    const uint32_t c1 = 0xcc9e2d51u, c2 = 0x1b873593u;
    uint32_t h = seed;
    uint64_t nblocks = len / 4;
    for (uint64_t i = 0; i < nblocks; i++) {
        uint32_t k;
        __builtin_memcpy(&k, key + i * 4, 4); /* little-endian */
        k *= c1;
        k = rotl32(k, 15);
        k *= c2;
        h ^= k;
        h = rotl32(h, 13);
        h = h * 5 + 0xe6546b64u;
    }
    uint32_t k1 = 0;
    const uint8_t* tail = key + nblocks * 4;
    switch (len & 3) {
        case 3: k1 ^= (uint32_t)tail[2] << 16; /* fallthrough */
        case 2: k1 ^= (uint32_t)tail[1] << 8;  /* fallthrough */
        case 1:
            k1 ^= tail[0];
            k1 *= c1;
            k1 = rotl32(k1, 15);
            k1 *= c2;
            h ^= k1;
    }
    h ^= (uint32_t)len;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

/* host-callable export so the CPU test suite can pin the restatement
 * against the published MurmurHash3 vectors without a GPU */
extern "C" uint32_t dbeel_murmur3_32(const uint8_t* key, uint64_t len,
                                     uint32_t seed) {
    return murmur3_32(key, len, seed);
}

/* between_cmp restated EXACTLY (tasks/migration.rs:54-60). Note the
 * reference's wrapped case (end < start) evaluates true for every hash —
 * restated verbatim, divergence-free. */
__device__ __forceinline__ bool hash_between(uint32_t h, uint32_t start,
                                             uint32_t end) {
    if (end < start) return h < start || h >= end;
    return h >= start && h < end;
}

__global__ void k_scanflag(RunsDesc R, const uint8_t* kbounds,
                           uint64_t start_len, uint64_t end_len,
                           int have_start, int have_end,
                           const uint32_t* rstart, const uint32_t* rend,
                           uint32_t n_ranges, RankRec* rrec,
                           uint32_t* err) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         g < R.total; g += stride) {
        int r = run_of(R, g);
        uint64_t i = g - R.entry_base[r];
        EView e;
        if (!load_entry(R, r, i, e)) {
            atomicOr(err, DERR_CORRUPT);
            RankRec z = {0, 8, 32};
            rrec[g] = z;
            continue;
        }
        bool keep = true;
        if (have_start &&
            cmp_keys(e.key, e.klen, kbounds, start_len) < 0)
            keep = false;
        if (keep && have_end &&
            cmp_keys(e.key, e.klen, kbounds + start_len, end_len) >= 0)
            keep = false;
        if (keep && n_ranges) {
            uint32_t h = murmur3_32(e.key, e.klen, 0);
            bool in_any = false;
            for (uint32_t j = 0; j < n_ranges && !in_any; j++)
                in_any = hash_between(h, rstart[j], rend[j]);
            keep = in_any;
        }
        RankRec m;
        m.src = ((uint64_t)r << 48) | e.off | (keep ? RR_KEEP : 0);
        m.key_size = e.key_size;
        m.full_size = e.full_size;
        rrec[g] = m; /* dense: rank == g (yield order, no reordering) */
    }
}

extern "C" int dbeel_gpu_scan(const dbeel_run_view* runs, size_t n_runs,
                              const uint8_t* start_key,
                              size_t start_key_len, const uint8_t* end_key,
                              size_t end_key_len,
                              const uint32_t* range_starts,
                              const uint32_t* range_ends, size_t n_ranges,
                              int device, dbeel_compact_result* out) {
    g_err[0] = 0;
    if (!out || (n_ranges && (!range_starts || !range_ends)) ||
        (start_key_len && !start_key) || (end_key_len && !end_key)) {
        set_err("scan: null argument");
        return DBEEL_ERR_INVALID_ARG;
    }
    dbeel_gpu_job* job = nullptr;
    int rc = dbeel_gpu_job_create(runs, n_runs, device, &job);
    if (rc) return rc;
    hipStream_t s = job->stream;
    uint64_t n = job->total_entries;

    uint8_t* d_kb = nullptr;
    uint32_t* d_ranges = nullptr;
    hipError_t e = hipSuccess;
    uint64_t kb_len = start_key_len + end_key_len;
    if (kb_len == 0) kb_len = 1;
    e = hipMalloc(&d_kb, kb_len);
    if (e == hipSuccess && start_key_len)
        e = hipMemcpyAsync(d_kb, start_key, start_key_len,
                           hipMemcpyHostToDevice, s);
    if (e == hipSuccess && end_key_len)
        e = hipMemcpyAsync(d_kb + start_key_len, end_key, end_key_len,
                           hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMalloc(&d_ranges, (n_ranges ? 2 * n_ranges : 1) * 4);
    if (e == hipSuccess && n_ranges) {
        e = hipMemcpyAsync(d_ranges, range_starts, n_ranges * 4,
                           hipMemcpyHostToDevice, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(d_ranges + n_ranges, range_ends,
                               n_ranges * 4, hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess)
        e = hipMemsetAsync(job->d_err, 0, 8, s);
    if (e == hipSuccess && n) {
        hipLaunchKernelGGL(k_scanflag, dim3(pick_grid(n, 256)), dim3(256),
                           0, s, job->desc, d_kb, (uint64_t)start_key_len,
                           (uint64_t)end_key_len, start_key ? 1 : 0,
                           end_key ? 1 : 0, d_ranges,
                           d_ranges + n_ranges, (uint32_t)n_ranges,
                           job->d_rank, job->d_err);
        size_t tmp = job->scantmp_bytes;
        e = survivor_scans(job->d_scantmp, tmp, job->d_rank, job->d_dstoff,
                           job->d_pos, n, s);
    }
    if (e == hipSuccess && n) {
        hipLaunchKernelGGL(k_emit, dim3(pick_grid(n, 256)), dim3(256), 0,
                           s, job->desc, job->d_rank, job->d_dstoff,
                           job->d_pos, n, job->d_outindex, job->d_srcmap,
                           job->d_err, job->d_tot);
        launch_copy(s, job->d_outindex, job->d_srcmap, job->d_winp0,
                    job->d_tot, n, job->total_data_bytes, job->d_outdata);
    } else if (e == hipSuccess) {
        e = hipMemsetAsync(job->d_tot, 0, sizeof(StepTotals), s);
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(job->h_tot, job->d_tot, sizeof(StepTotals),
                           hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipGetLastError();

    job->last_scan_packed = 0;
    int ret = DBEEL_OK;
    if (e != hipSuccess) {
        set_err("scan failed: %s", hipGetErrorString(e));
        ret = DBEEL_ERR_HIP;
    } else if (job->h_tot->err) {
        set_err("corrupt entry/index record");
        ret = DBEEL_ERR_CORRUPT;
    } else {
        job->out_data_len = job->h_tot->total_out;
        job->out_entries = job->h_tot->n_surv;
        job->have_result = true;
        ret = dbeel_gpu_job_fetch(job, out);
    }
    hipFree(d_kb);
    hipFree(d_ranges);
    dbeel_gpu_job_destroy(job);
    return ret;
}

/* ------------------------------------------------------------------ */
/* Paged scan over the resident tables (dbeel_gpu_reader_scan_*)      */
/*                                                                    */
/* dbeel_gpu_scan above loads every entry of every run, whatever the  */
/* key range. Here the key range is resolved ONCE, per table, on the  */
/* resident prefix arrays (k_reader_scan_bounds): the candidates are  */
/* the concatenation over tables of [lower_bound(start),              */
/* lower_bound(end)), and a page is a window of that space:           */
/*   k_reader_scan_flag : candidate -> (table, entry); hash filter +  */
/*                        first matching range; one RankRec + range   */
/*                        id per candidate. No key compares.          */
/*   rocPRIM scans      : survivor byte offsets and positions inside  */
/*                        the window (the job pipeline's functors).   */
/*   k_reader_scan_emit : capped emit — the survivors that fit the    */
/*                        caller's data / index capacity form a       */
/*                        prefix; index records, source addresses and */
/*                        compacted range ids for those, plus the     */
/*                        page totals and the next cursor position.   */
/*   k_winmap / k_copy  : unchanged, into the reader's page buffer.   */
/* ------------------------------------------------------------------ */

/* Candidate space -> table entries, by value next to RunsDesc: table r
 * owns the candidates [cend[r-1], cend[r]) and candidate c of it is entry
 * c + adj[r] (adj = first in-range entry minus the table's candidate base,
 * modulo 2^64). */
struct ScanWin {
    uint64_t cend[MAX_RUNS];
    uint64_t adj[MAX_RUNS];
};
static_assert(sizeof(RunsDesc) + sizeof(ScanWin) + 128 <= 4096,
              "k_reader_scan_flag arguments must fit the kernarg segment");

#define SCAN_NO_RANGE 0xFFFFFFFFu
#define SCAN_DEFAULT_CANDIDATES (1ull << 20)
#define SCAN_MAX_CANDIDATES (1ull << 31) /* survivor positions are u32 */

/* One thread per (table, bound): bounds[2r] = lower_bound(start_key),
 * bounds[2r+1] = lower_bound(end_key) in table r; an absent bound gives 0 /
 * count. k_reader_search's shape: bisect the prefixes, then settle the
 * equal-prefix stretch (zero padding, bytes past 8, length) by a second
 * bisection with full key compares on the blob — never a walk. */
__global__ void k_reader_scan_bounds(RunsDesc R, ReaderPfx pfx,
                                     const uint8_t* kbounds,
                                     uint64_t start_len, uint64_t end_len,
                                     int have_start, int have_end,
                                     uint64_t* bounds) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2u * (uint32_t)R.n_runs) return;
    const int r = (int)(t >> 1);
    const bool is_end = t & 1;
    const uint64_t n = R.count[r];
    if (!(is_end ? have_end : have_start)) {
        bounds[t] = is_end ? n : 0;
        return;
    }
    const uint8_t* key = is_end ? kbounds + start_len : kbounds;
    const uint64_t klen = is_end ? end_len : start_len;
    const uint64_t qp = key_prefix(key, klen);
    const uint64_t* P = pfx.p[r];
    const uint64_t lo = pfx_lower_bound(P, n, qp);
    const uint64_t end = pfx_upper_bound(P, lo, n, qp);
    /* [lo, end) share the bound's prefix and are in key order: the first
     * one >= the bound is the answer (end when there is none) */
    bounds[t] = blob_lower_bound(R, r, lo, end, key, klen);
}

__global__ void k_reader_scan_flag(RunsDesc R, ScanWin W, uint64_t c0,
                                   uint64_t m, const uint32_t* rstart,
                                   const uint32_t* rend, uint32_t n_ranges,
                                   RankRec* rrec, uint32_t* rid) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < m;
         w += stride) {
        const uint64_t c = c0 + w;
        int r = 0;
        while (r + 1 < R.n_runs && c >= W.cend[r]) r++;
        const uint64_t i = c + W.adj[r];
        EView e;
        if (i >= R.count[r] || !load_entry(R, r, i, e)) {
            /* cannot happen on tables validated at open; stay memory safe */
            RankRec z = {0, 8, 32};
            rrec[w] = z;
            rid[w] = SCAN_NO_RANGE;
            continue;
        }
        uint32_t id = SCAN_NO_RANGE;
        if (n_ranges) {
            const uint32_t h = murmur3_32(e.key, e.klen, 0);
            for (uint32_t j = 0; j < n_ranges; j++)
                if (hash_between(h, rstart[j], rend[j])) {
                    id = j;
                    break;
                }
        }
        const bool keep = n_ranges == 0 || id != SCAN_NO_RANGE;
        RankRec rec;
        rec.src = ((uint64_t)r << 48) | e.off | (keep ? RR_KEEP : 0);
        rec.key_size = e.key_size;
        rec.full_size = e.full_size;
        rrec[w] = rec;
        rid[w] = id;
    }
}

/* Does everything up to AND INCLUDING window position g fit the page?
 * off / pos are the exclusive survivor sums at g. Both sums only grow with
 * g, so the positions that fit form a prefix of the window. */
__device__ __forceinline__ bool scan_page_fits(const RankRec& m, uint64_t off,
                                               uint32_t pos,
                                               uint64_t data_cap,
                                               uint64_t max_entries) {
    const bool kept = m.src & RR_KEEP;
    return off + (kept ? m.full_size : 0u) <= data_cap &&
           (uint64_t)pos + (kept ? 1u : 0u) <= max_entries;
}

/* Capped emit. Exactly one thread owns the page totals: the last position
 * that fits (its successor, if any, is then a survivor that does not), or
 * position 0 when not even that fits. Plain vector stores, no atomics. */
__global__ void k_reader_scan_emit(RunsDesc R, const RankRec* rrec,
                                   const uint32_t* rid,
                                   const uint64_t* dst_off,
                                   const uint32_t* pos, uint64_t m,
                                   uint64_t data_cap, uint64_t max_entries,
                                   uint8_t* out_index, uint64_t* src_map,
                                   uint32_t* rid_out, ScanPageTotals* tot) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < m;
         g += stride) {
        const RankRec rec = rrec[g];
        const uint64_t off = dst_off[g];
        const uint32_t p = pos[g];
        if (!scan_page_fits(rec, off, p, data_cap, max_entries)) {
            if (g == 0) {
                tot->st.total_out = 0;
                tot->st.n_surv = 0;
                tot->st.err = 0;
                tot->next = 0;
                tot->next_full = rec.full_size;
            }
            continue;
        }
        const bool kept = rec.src & RR_KEEP;
        bool last = g + 1 == m;
        uint64_t next_full = 0;
        if (!last) {
            const RankRec nx = rrec[g + 1];
            last = !scan_page_fits(nx, dst_off[g + 1], pos[g + 1], data_cap,
                                   max_entries);
            next_full = nx.full_size;
        }
        if (last) {
            tot->st.total_out = off + (kept ? rec.full_size : 0u);
            tot->st.n_surv = (uint64_t)p + (kept ? 1u : 0u);
            tot->st.err = 0;
            tot->next = g + 1;
            tot->next_full = next_full;
        }
        if (!kept) continue;
        uint8_t* out = out_index + (uint64_t)p * 16;
        __builtin_memcpy(out, &off, 8);
        __builtin_memcpy(out + 8, &rec.key_size, 4);
        __builtin_memcpy(out + 12, &rec.full_size, 4);
        src_map[p] = (uint64_t)(R.data[(rec.src >> 48) & 0x7FFF] +
                                (rec.src & RR_OFF_MASK));
        rid_out[p] = rid[g];
    }
}

/* ---- DBEEL_SCAN_NEWEST_ONLY: the shadow pass ----
 * Runs between k_reader_scan_flag and the survivor scans and clears RR_KEEP
 * on every kept window record whose key a LATER segment of the snapshot
 * holds: the memtable first (a ReaderMem leg like mem_search), then tables
 * n-1 .. r+1, stopping at the first match. Each table probe has
 * k_reader_search's shape — filter check with the hash pair computed once
 * per seed, bisection of the dense prefix array, then the equal-prefix
 * stretch settled by bisection with full key compares, never a walk.
 *
 * NARROW (DBEEL_SCAN_SHADOW=narrow; not the default — it measured level
 * with the plain pass): the window's candidates are consecutive entries of sorted tables,
 * so a tile of SHADOW_BLOCK consecutive candidates of ONE table can only
 * match inside [lower_bound(prefix of its first key), upper_bound(prefix of
 * its last key)) of each later segment. One thread per later segment (at
 * most 64 tables + the memtable) bisects those two bounds into LDS once per
 * tile, and every lane then bisects the narrowed slice only. A tile that
 * straddles a table boundary, and a lane whose prefix lies outside the
 * tile's bounds, use the full bisection. LDS: 65 * 16 B = 1040 B per block;
 * at 256 threads the block's occupancy is set by registers, not LDS. */
#define SHADOW_BLOCK 256
#define SHADOW_SEGS (MAX_RUNS + 1) /* slot MAX_RUNS = the memtable */

/* Is (key, klen) in table r? Prefix bisection confined to [blo, bhi). */
__device__ __forceinline__ bool table_has_key(const RunsDesc& R,
                                              const uint64_t* P, int r,
                                              uint64_t blo, uint64_t bhi,
                                              const uint8_t* key,
                                              uint64_t klen, uint64_t qp) {
    uint64_t lo = blo + pfx_lower_bound(P + blo, bhi - blo, qp);
    if (lo >= bhi || P[lo] != qp) return false;
    uint64_t end = lo + 1;
    if (end < bhi && P[end] == qp) end = pfx_upper_bound(P, end + 1, bhi, qp);
    while (lo < end) {
        const uint64_t mid = (lo + end) >> 1;
        EView m;
        if (!load_entry(R, r, mid, m)) { /* validated at open */
            end = mid;
            continue;
        }
        const int cmp = cmp_keys(m.key, m.klen, key, klen);
        if (cmp == 0) return true;
        if (cmp < 0)
            lo = mid + 1;
        else
            end = mid;
    }
    return false;
}

template <bool NARROW>
__global__ __launch_bounds__(SHADOW_BLOCK) void k_reader_scan_shadow(
    RunsDesc R, ReaderPfx pfx, ReaderMem mem, const ReaderBloom* blooms,
    uint64_t m, RankRec* rrec) {
    __shared__ uint64_t s_lo[SHADOW_SEGS], s_hi[SHADOW_SEGS];
    __shared__ int s_tile_run; /* the tile's table, -1 = straddles */
    __shared__ uint64_t s_pf, s_pl;
    const uint64_t n_tiles = (m + SHADOW_BLOCK - 1) / SHADOW_BLOCK;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t w0 = tile * SHADOW_BLOCK;
        const uint64_t w = w0 + threadIdx.x;
        if constexpr (NARROW) {
            __syncthreads(); /* the previous tile's bounds are done with */
            const uint64_t wl =
                (w0 + SHADOW_BLOCK <= m ? w0 + SHADOW_BLOCK : m) - 1;
            const RankRec a = rrec[w0], z = rrec[wl];
            const int ra = (int)((a.src >> 48) & 0x7FFF);
            const int rz = (int)((z.src >> 48) & 0x7FFF);
            const uint64_t pf = key_prefix(
                R.data[ra] + (a.src & RR_OFF_MASK) + 8, a.key_size - 8);
            const uint64_t pl = key_prefix(
                R.data[rz] + (z.src & RR_OFF_MASK) + 8, z.key_size - 8);
            if (threadIdx.x == 0) {
                s_tile_run = ra == rz ? ra : -1;
                s_pf = pf;
                s_pl = pl;
            }
            const int t = (int)threadIdx.x;
            if (ra == rz && t < SHADOW_SEGS) {
                const uint64_t* P = nullptr;
                uint64_t n = 0;
                if (t == MAX_RUNS) {
                    P = mem.pfx;
                    n = mem.count;
                } else if (t > ra && t < R.n_runs) {
                    P = pfx.p[t];
                    n = R.count[t];
                }
                uint64_t lo = 0, hi = 0;
                if (n) {
                    lo = pfx_lower_bound(P, n, pf);
                    hi = pfx_upper_bound(P, lo, n, pl);
                }
                s_lo[t] = lo;
                s_hi[t] = hi;
            }
            __syncthreads();
        }
        if (w >= m) continue;
        const RankRec rec = rrec[w];
        if (!(rec.src & RR_KEEP)) continue;
        const int r = (int)((rec.src >> 48) & 0x7FFF);
        const uint8_t* key = R.data[r] + (rec.src & RR_OFF_MASK) + 8;
        const uint64_t klen = rec.key_size - 8;
        const uint64_t qp = key_prefix(key, klen);
        bool narrow = false;
        if constexpr (NARROW)
            narrow = s_tile_run == r && qp >= s_pf && qp <= s_pl;
        bool shadowed = false;
        if (mem.count) {
            uint64_t off, vlen;
            if (narrow) {
                /* the index records hold offsets into data: a slice of the
                 * index and prefix arrays is a memtable of its own */
                const uint64_t lo = s_lo[MAX_RUNS], hi = s_hi[MAX_RUNS];
                const ReaderMem sl = {mem.data, mem.index + lo * 16,
                                      mem.pfx + lo, hi - lo};
                shadowed = mem_search(sl, key, klen, qp, off, vlen);
            } else {
                shadowed = mem_search(mem, key, klen, qp, off, vlen);
            }
        }
        bool have_hash = false;
        uint64_t hseed = 0, h1 = 0, h2 = 0;
        for (int t = R.n_runs - 1; t > r && !shadowed; t--) {
            const uint64_t n = R.count[t];
            uint64_t blo = 0, bhi = n;
            if (narrow) {
                blo = s_lo[t];
                bhi = s_hi[t];
            }
            if (blo >= bhi) continue;
            const ReaderBloom B = blooms[t];
            if (B.bits) {
                if (!have_hash || hseed != B.seed) {
                    hseed = B.seed;
                    h1 = d_fnv1a64(key, klen, hseed);
                    h2 = d_fnv1a64(key, klen,
                                   hseed ^ 0x9e3779b97f4a7c15ull) | 1;
                    have_hash = true;
                }
                bool maybe = true;
                for (uint32_t j = 0; j < B.k; j++) {
                    const uint64_t bit = (h1 + j * h2) % B.n_bits;
                    if (!(B.bits[bit >> 3] & (1u << (bit & 7)))) {
                        maybe = false;
                        break;
                    }
                }
                if (!maybe) continue;
            }
            shadowed = table_has_key(R, pfx.p[t], t, blo, bhi, key, klen, qp);
        }
        if (shadowed) rrec[w].src = rec.src & ~RR_KEEP;
    }
}

/* Shadowed candidates among the first tot->next of the window — the ones
 * the page consumed; the caps may cut a window short, and what lies past
 * the cut is examined again by the next page. A candidate that passed the
 * hash filter and is not kept was cleared by the shadow pass. Block
 * reduction, then one atomic per block. */
__global__ __launch_bounds__(256) void k_reader_scan_shadow_count(
    const RankRec* rrec, const uint32_t* rid, uint32_t n_ranges,
    ScanPageTotals* tot) {
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const uint64_t n = tot->next;
    unsigned long long c = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n;
         g += stride)
        if (!(rrec[g].src & RR_KEEP) &&
            (n_ranges == 0 || rid[g] != SCAN_NO_RANGE))
            c++;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_sum, c);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum)
        atomicAdd((unsigned long long*)&tot->shadowed, s_sum);
}

struct dbeel_gpu_reader_scan {
    dbeel_gpu_reader* rd = nullptr;
    uint64_t generation = 0; /* rd->generation at begin */
    ScanWin win{};
    uint64_t total = 0;  /* candidates in all segments */
    uint64_t cursor = 0; /* next candidate to examine */
    uint64_t max_candidates = 0;
    uint32_t* d_ranges = nullptr; /* starts | ends */
    uint32_t n_ranges = 0;
    uint32_t n_tables = 0;        /* tables in the list at begin */
    uint64_t table_total = 0;     /* candidates in the tables */
    /* snapshot scans (dbeel_gpu_reader_scan_snapshot): what the kernels saw
     * of the list at begin, a reference to every table of it, and — with
     * DBEEL_SCAN_MEMTABLE and a non-empty memtable — the memtable of that
     * moment as the last segment: candidates [table_total, total), entry
     * mem_lo + (c - table_total). Nothing here follows a list edit. */
    bool snapshot = false;
    uint32_t flags = 0;
    RunsDesc desc{};
    ReaderPfx pfx{};
    ReaderBloom* d_blooms = nullptr; /* NEWEST_ONLY: the filters at begin */
    std::vector<ReaderTable> held;
    MemHold* mem_hold = nullptr;
    ReaderMem mem{};
    uint64_t mem_data_len = 0, mem_lo = 0;
    uint64_t shadowed = 0;
};

static void scan_free(dbeel_gpu_reader_scan* sc) {
    (void)hipFree(sc->d_ranges);
    (void)hipFree(sc->d_blooms);
    for (ReaderTable& t : sc->held) table_free(t);
    if (MemHold* h = sc->mem_hold) {
        if (--h->refs == 0) {
            if (h->in_pair) {
                for (ReaderMemtable::Buf& b : sc->rd->mem.buf)
                    if (b.hold == h) b.hold = nullptr;
            } else {
                (void)hipFree(h->d_run);
                (void)hipFree(h->d_pfx);
            }
            delete h;
        }
    }
    delete sc;
}

extern "C" uint64_t dbeel_gpu_reader_held_bytes(const dbeel_gpu_reader* rd) {
    if (!rd) return 0;
    /* each buffer once, however many scans hold it */
    std::vector<const void*> seen;
    uint64_t sum = 0;
    auto first_time = [&](const void* p) {
        for (const void* q : seen)
            if (q == p) return false;
        seen.push_back(p);
        return true;
    };
    for (const ReaderTable& t : rd->tables) seen.push_back(t.d_run);
    for (const dbeel_gpu_reader_scan* sc : rd->scans) {
        for (const ReaderTable& t : sc->held)
            if (first_time(t.d_run)) sum += t.bytes;
        const MemHold* h = sc->mem_hold;
        if (h && !h->in_pair && first_time(h)) sum += h->bytes;
    }
    return sum;
}

extern "C" int dbeel_gpu_reader_scan_info(const dbeel_gpu_reader_scan* sc,
                                          dbeel_scan_snapshot_info* info) {
    g_err[0] = 0;
    if (info) memset(info, 0, sizeof *info);
    if (!sc || !info) {
        set_err("reader_scan_info: null argument");
        return DBEEL_ERR_INVALID_ARG;
    }
    info->n_tables = sc->n_tables;
    info->has_memtable = sc->mem.count ? 1 : 0;
    info->table_candidates = sc->table_total;
    info->memtable_candidates = sc->total - sc->table_total;
    info->shadowed = sc->shadowed;
    return DBEEL_OK;
}

static void reader_end_scans(dbeel_gpu_reader* rd) {
    for (dbeel_gpu_reader_scan* sc : rd->scans) scan_free(sc);
    rd->scans.clear();
}

extern "C" void dbeel_gpu_reader_scan_end(dbeel_gpu_reader_scan* sc) {
    if (!sc) return;
    dbeel_gpu_reader* rd = sc->rd;
    if (rd->device >= 0) (void)hipSetDevice(rd->device);
    for (size_t i = 0; i < rd->scans.size(); i++)
        if (rd->scans[i] == sc) {
            rd->scans.erase(rd->scans.begin() + i);
            break;
        }
    scan_free(sc);
}

/* begin of both kinds of scan; fn names the entry point in messages. The
 * checks are host-only and come before any device call. */
static int scan_begin_impl(const char* fn, bool snapshot, uint32_t flags,
    dbeel_gpu_reader* rd, const uint8_t* start_key, size_t start_key_len,
    const uint8_t* end_key, size_t end_key_len, const uint32_t* range_starts,
    const uint32_t* range_ends, size_t n_ranges, uint64_t max_candidates,
    dbeel_gpu_reader_scan** out) {
    if (!rd || !out) {
        set_err("%s: null reader or out", fn);
        return DBEEL_ERR_INVALID_ARG;
    }
    if ((start_key_len && !start_key) || (end_key_len && !end_key)) {
        set_err("%s: key length given without its pointer", fn);
        return DBEEL_ERR_INVALID_ARG;
    }
    if (n_ranges && (!range_starts || !range_ends)) {
        set_err("%s: n_ranges given without the range arrays", fn);
        return DBEEL_ERR_INVALID_ARG;
    }
    if (n_ranges >= SCAN_NO_RANGE) {
        set_err("%s: too many hash ranges", fn);
        return DBEEL_ERR_INVALID_ARG;
    }
    HIP_CHECK(hipSetDevice(rd->device));
    hipStream_t s = rd->stream;
    if (!rd->d_scantot)
        HIP_CHECK(hipMalloc(&rd->d_scantot, sizeof(ScanPageTotals)));
    if (!rd->h_scantot)
        HIP_CHECK(hipHostMalloc(&rd->h_scantot, sizeof(ScanPageTotals)));
    dbeel_gpu_reader_scan* sc = new (std::nothrow) dbeel_gpu_reader_scan();
    if (!sc) {
        set_err("host alloc failed");
        return DBEEL_ERR_OOM;
    }
    sc->rd = rd;
    sc->generation = rd->generation;
    sc->n_ranges = (uint32_t)n_ranges;
    sc->max_candidates = max_candidates ? max_candidates
                                        : SCAN_DEFAULT_CANDIDATES;
    if (sc->max_candidates > SCAN_MAX_CANDIDATES)
        sc->max_candidates = SCAN_MAX_CANDIDATES;
    sc->snapshot = snapshot;
    sc->flags = flags;

    const int n_runs = rd->desc.n_runs;
    sc->n_tables = (uint32_t)n_runs;
    const bool want_mem =
        snapshot && (flags & DBEEL_SCAN_MEMTABLE) && rd->mem.count;
    /* host allocations of the snapshot come first: past them only device
     * calls can fail, and those change nothing of the reader */
    MemHold* new_hold = nullptr;
    if (snapshot) {
        bool ok = true;
        try {
            sc->held.reserve(rd->tables.size());
        } catch (...) {
            ok = false;
        }
        for (ReaderTable& t : rd->tables)
            if (ok && !t.refs) {
                t.refs = new (std::nothrow) uint32_t(1); /* the list */
                ok = t.refs != nullptr;
            }
        if (ok && want_mem && !rd->mem.buf[rd->mem.cur].hold) {
            new_hold = new (std::nothrow) MemHold();
            ok = new_hold != nullptr;
        }
        if (!ok) {
            set_err("host alloc failed");
            scan_free(sc);
            return DBEEL_ERR_OOM;
        }
    }
    const uint64_t kb_len = (uint64_t)start_key_len + end_key_len;
    uint64_t hb[2 * MAX_RUNS + 2]; /* tables, then the memtable segment */
    uint8_t* d_kb = nullptr; /* bound keys | the bounds, 8-B aligned */
    const uint64_t kb_pad = (kb_len + 7) & ~7ull;
    hipError_t e = hipSuccess;
    if (n_ranges) {
        e = hipMalloc(&sc->d_ranges, 2 * n_ranges * sizeof(uint32_t));
        if (e == hipSuccess)
            e = hipMemcpyAsync(sc->d_ranges, range_starts, n_ranges * 4,
                               hipMemcpyHostToDevice, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(sc->d_ranges + n_ranges, range_ends,
                               n_ranges * 4, hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess && snapshot && (flags & DBEEL_SCAN_NEWEST_ONLY)) {
        /* rd->d_blooms is rewritten by every list edit */
        e = hipMalloc(&sc->d_blooms, MAX_RUNS * sizeof(ReaderBloom));
        if (e == hipSuccess)
            e = hipMemcpyAsync(sc->d_blooms, rd->d_blooms,
                               MAX_RUNS * sizeof(ReaderBloom),
                               hipMemcpyDeviceToDevice, s);
    }
    if (e == hipSuccess && (n_runs || want_mem)) {
        e = hipMalloc(&d_kb, kb_pad + sizeof hb);
        if (e == hipSuccess && start_key_len)
            e = hipMemcpyAsync(d_kb, start_key, start_key_len,
                               hipMemcpyHostToDevice, s);
        if (e == hipSuccess && end_key_len)
            e = hipMemcpyAsync(d_kb + start_key_len, end_key, end_key_len,
                               hipMemcpyHostToDevice, s);
        uint64_t* d_bounds = (uint64_t*)(d_kb + kb_pad);
        if (e == hipSuccess && n_runs) {
            hipLaunchKernelGGL(k_reader_scan_bounds, dim3(1),
                               dim3(2 * MAX_RUNS), 0, s, rd->desc, rd->pfx,
                               d_kb, (uint64_t)start_key_len,
                               (uint64_t)end_key_len, start_key ? 1 : 0,
                               end_key ? 1 : 0, d_bounds);
            e = hipMemcpyAsync(hb, d_bounds,
                               2 * (size_t)n_runs * sizeof(uint64_t),
                               hipMemcpyDeviceToHost, s);
        }
        if (e == hipSuccess && want_mem) {
            /* the memtable segment's bounds: the same bisection over its
             * own prefix array, as a table list of one */
            const ReaderMemtable& M = rd->mem;
            RunsDesc D1;
            memset(&D1, 0, sizeof D1);
            D1.n_runs = 1;
            D1.total = M.count;
            D1.data[0] = M.data();
            D1.index[0] = M.index();
            D1.data_len[0] = M.data_len;
            D1.count[0] = M.count;
            D1.job_hi[0] = 1;
            ReaderPfx P1;
            memset(&P1, 0, sizeof P1);
            P1.p[0] = M.buf[M.cur].d_pfx;
            hipLaunchKernelGGL(k_reader_scan_bounds, dim3(1),
                               dim3(2 * MAX_RUNS), 0, s, D1, P1, d_kb,
                               (uint64_t)start_key_len, (uint64_t)end_key_len,
                               start_key ? 1 : 0, end_key ? 1 : 0,
                               d_bounds + 2 * MAX_RUNS);
            e = hipMemcpyAsync(hb + 2 * MAX_RUNS, d_bounds + 2 * MAX_RUNS,
                               2 * sizeof(uint64_t), hipMemcpyDeviceToHost,
                               s);
        }
    }
    /* the caller's keys and ranges are read by the async copies above */
    hipError_t se = hipStreamSynchronize(s);
    if (e == hipSuccess) e = se;
    if (e == hipSuccess) e = hipGetLastError();
    (void)hipFree(d_kb);
    if (e != hipSuccess) {
        set_err("%s: %s", fn, hipGetErrorString(e));
        delete new_hold;
        scan_free(sc);
        return e == hipErrorOutOfMemory ? DBEEL_ERR_OOM : DBEEL_ERR_HIP;
    }
    uint64_t base = 0;
    for (int r = 0; r < n_runs; r++) {
        uint64_t lo = hb[2 * r], hi = hb[2 * r + 1];
        const uint64_t n = rd->desc.count[r];
        if (lo > n) lo = n;
        if (hi > n) hi = n;
        if (hi < lo) hi = lo; /* start > end: nothing */
        sc->win.adj[r] = lo - base;
        base += hi - lo;
        sc->win.cend[r] = base;
    }
    sc->table_total = base;
    if (snapshot) {
        /* nothing can fail from here: take the references */
        sc->desc = rd->desc;
        sc->pfx = rd->pfx;
        for (ReaderTable& t : rd->tables) {
            ++*t.refs;
            sc->held.push_back(t);
        }
    }
    if (want_mem) {
        ReaderMemtable& M = rd->mem;
        ReaderMemtable::Buf& cur = M.buf[M.cur];
        if (!cur.hold) {
            new_hold->d_run = cur.d_run;
            new_hold->d_pfx = cur.d_pfx;
            cur.hold = new_hold;
        }
        cur.hold->refs++;
        sc->mem_hold = cur.hold;
        sc->mem = M.view();
        sc->mem_data_len = M.data_len;
        uint64_t lo = hb[2 * MAX_RUNS], hi = hb[2 * MAX_RUNS + 1];
        if (lo > M.count) lo = M.count;
        if (hi > M.count) hi = M.count;
        if (hi < lo) hi = lo;
        sc->mem_lo = lo;
        base += hi - lo;
    }
    sc->total = base;
    rd->scans.push_back(sc);
    *out = sc;
    return DBEEL_OK;
}

extern "C" int dbeel_gpu_reader_scan_begin(
    dbeel_gpu_reader* rd, const uint8_t* start_key, size_t start_key_len,
    const uint8_t* end_key, size_t end_key_len, const uint32_t* range_starts,
    const uint32_t* range_ends, size_t n_ranges, uint64_t max_candidates,
    dbeel_gpu_reader_scan** out) {
    g_err[0] = 0;
    if (out) *out = nullptr;
    return scan_begin_impl("reader_scan_begin", false, 0, rd, start_key,
                           start_key_len, end_key, end_key_len, range_starts,
                           range_ends, n_ranges, max_candidates, out);
}

extern "C" int dbeel_gpu_reader_scan_snapshot(
    dbeel_gpu_reader* rd, const uint8_t* start_key, size_t start_key_len,
    const uint8_t* end_key, size_t end_key_len, const uint32_t* range_starts,
    const uint32_t* range_ends, size_t n_ranges, uint64_t max_candidates,
    uint32_t flags, dbeel_gpu_reader_scan** out) {
    g_err[0] = 0;
    if (out) *out = nullptr;
    if (flags & ~(uint32_t)(DBEEL_SCAN_MEMTABLE | DBEEL_SCAN_NEWEST_ONLY)) {
        set_err("reader_scan_snapshot: unknown flags 0x%x (defined: "
                "DBEEL_SCAN_MEMTABLE, DBEEL_SCAN_NEWEST_ONLY)", flags);
        return DBEEL_ERR_INVALID_ARG;
    }
    return scan_begin_impl("reader_scan_snapshot", true, flags, rd, start_key,
                           start_key_len, end_key, end_key_len, range_starts,
                           range_ends, n_ranges, max_candidates, out);
}

static inline uint64_t scan_align16(uint64_t v) { return (v + 15) & ~15ull; }

/* One page as drawn on the device, before anything is committed: the
 * entries lie in rd->d_page, their records and range ids in the scan
 * scratch, until the reader's next page. */
struct ScanDrawn {
    uint64_t taken, bytes, next; /* entries | data bytes | candidates */
    bool shadow, done;           /* done: nothing was left to draw    */
    const uint8_t* d_oidx;
    const uint32_t* d_rido;
    float ms[3];                 /* flag | emit | copy */
};

/* Draws the next page for scan_next and scan_apply (fn names the entry
 * point in messages): everything up to and including the ITEM_TOO_LARGE
 * verdict, with rd->stream idle on return and the cursor untouched. The
 * stale check is the caller's. */
static int scan_draw(const char* fn, dbeel_gpu_reader_scan* sc,
                     uint64_t data_cap, uint64_t index_cap,
                     dbeel_scan_page* page, ScanDrawn& out) {
    dbeel_gpu_reader* rd = sc->rd;
    memset(&out, 0, sizeof out);
    /* a page is cut from ONE descriptor: the tables' (at most 64 runs), or
     * — once they are exhausted — the memtable segment's, a list of one.
     * The page that exhausts the tables may therefore be short. */
    const bool mem_page = sc->cursor >= sc->table_total;
    uint64_t m = (mem_page ? sc->total : sc->table_total) - sc->cursor;
    if (m > sc->max_candidates) m = sc->max_candidates;
    if (m == 0) {
        page->done = 1;
        out.done = true;
        return DBEEL_OK;
    }
    RunsDesc mem_desc;
    ScanWin mem_win;
    if (mem_page) {
        memset(&mem_desc, 0, sizeof mem_desc);
        mem_desc.n_runs = 1;
        mem_desc.total = sc->mem.count;
        mem_desc.data[0] = sc->mem.data;
        mem_desc.index[0] = sc->mem.index;
        mem_desc.data_len[0] = sc->mem_data_len;
        mem_desc.count[0] = sc->mem.count;
        mem_desc.job_hi[0] = 1;
        memset(&mem_win, 0, sizeof mem_win);
        mem_win.cend[0] = sc->total - sc->table_total;
        mem_win.adj[0] = sc->mem_lo;
    }
    const RunsDesc& D =
        mem_page ? mem_desc : (sc->snapshot ? sc->desc : rd->desc);
    const ScanWin& W = mem_page ? mem_win : sc->win;
    const uint64_t c0 = mem_page ? sc->cursor - sc->table_total : sc->cursor;
    /* nothing follows the memtable: its pages skip the shadow pass */
    const bool shadow =
        !mem_page && sc->snapshot && (sc->flags & DBEEL_SCAN_NEWEST_ONLY);
    bool shadow_narrow = false;
    if (shadow) {
        /* read on every call, as DBEEL_BATCH_ORDER is; "full" is the
         * default: the narrowed pass measured level with it (DESIGN.md
         * §4b-7) */
        const char* v = getenv("DBEEL_SCAN_SHADOW");
        if (v && !strcmp(v, "narrow")) shadow_narrow = true;
    }
    uint64_t resident = 0; /* no page can hold more than the tables do */
    for (int r = 0; r < D.n_runs; r++) resident += D.data_len[r];
    const uint64_t cap = data_cap < resident ? (uint64_t)data_cap : resident;
    uint64_t max_entries = index_cap / 16;
    if (max_entries > m) max_entries = m;

    /* scratch: rrec | dst_off | pos | rid | out_index | src_map | rid_out */
    const uint64_t o_rrec = 0;
    const uint64_t o_dst = o_rrec + m * sizeof(RankRec);
    const uint64_t o_pos = o_dst + scan_align16(m * 8);
    const uint64_t o_rid = o_pos + scan_align16(m * 4);
    const uint64_t o_oidx = o_rid + scan_align16(m * 4);
    const uint64_t o_smap = o_oidx + max_entries * 16;
    const uint64_t o_rido = o_smap + scan_align16(max_entries * 8);
    const uint64_t scratch = o_rido + scan_align16(max_entries * 4);

    hipStream_t s = rd->stream;
    /* on failure nothing of this page may still be in flight into the
     * caller's buffers or the shared scratch */
    ScopeGuard sync_on_fail([&] { (void)hipStreamSynchronize(s); });

    HIP_CHECK(hipSetDevice(rd->device));
    HIP_CHECK(reader_reserve((void**)&rd->d_scan, &rd->scan_cap, scratch));
    HIP_CHECK(reader_reserve((void**)&rd->d_page, &rd->page_cap,
                             scan_align16(cap ? cap : 16)));
    /* sized for the smallest copy-window variant (8 KiB) */
    HIP_CHECK(reader_reserve((void**)&rd->d_scanwin, &rd->scanwin_cap,
                             (cap / 8192 + 2) * sizeof(uint32_t)));
    RankRec* d_rrec = (RankRec*)(rd->d_scan + o_rrec);
    uint64_t* d_dst = (uint64_t*)(rd->d_scan + o_dst);
    uint32_t* d_pos = (uint32_t*)(rd->d_scan + o_pos);
    uint32_t* d_rid = (uint32_t*)(rd->d_scan + o_rid);
    uint8_t* d_oidx = rd->d_scan + o_oidx;
    uint64_t* d_smap = (uint64_t*)(rd->d_scan + o_smap);
    uint32_t* d_rido = (uint32_t*)(rd->d_scan + o_rido);
    size_t tmp_bytes = 0;
    HIP_CHECK(survivor_scans(nullptr, tmp_bytes, d_rrec, d_dst, d_pos, m, s));
    HIP_CHECK(reader_reserve(&rd->d_scantmp, &rd->scantmp_cap,
                             tmp_bytes ? tmp_bytes : 1));

    HIP_CHECK(hipEventRecord(rd->ev[0], s));
    hipLaunchKernelGGL(k_reader_scan_flag, dim3(pick_grid(m, 256)), dim3(256),
                       0, s, D, W, c0, m, sc->d_ranges,
                       sc->d_ranges + sc->n_ranges, sc->n_ranges, d_rrec,
                       d_rid);
    if (shadow) {
        const uint32_t tiles =
            (uint32_t)((m + SHADOW_BLOCK - 1) / SHADOW_BLOCK);
        hipLaunchKernelGGL(shadow_narrow ? k_reader_scan_shadow<true>
                                         : k_reader_scan_shadow<false>,
                           dim3(tiles < 65535u * 16 ? tiles : 65535u * 16),
                           dim3(SHADOW_BLOCK), 0, s, D, sc->pfx, sc->mem,
                           sc->d_blooms, m, d_rrec);
        HIP_CHECK(hipMemsetAsync(&rd->d_scantot->shadowed, 0, 8, s));
    }
    HIP_CHECK(hipEventRecord(rd->ev[1], s));
    HIP_CHECK(survivor_scans(rd->d_scantmp, tmp_bytes, d_rrec, d_dst, d_pos,
                             m, s));
    hipLaunchKernelGGL(k_reader_scan_emit, dim3(pick_grid(m, 256)), dim3(256),
                       0, s, D, d_rrec, d_rid, d_dst, d_pos, m,
                       (uint64_t)data_cap, max_entries, d_oidx, d_smap,
                       d_rido, rd->d_scantot);
    if (shadow)
        hipLaunchKernelGGL(k_reader_scan_shadow_count,
                           dim3(pick_grid(m, 256)), dim3(256), 0, s, d_rrec,
                           d_rid, sc->n_ranges, rd->d_scantot);
    HIP_CHECK(hipEventRecord(rd->ev[2], s));
    {
        /* the copy's grid comes from an upper bound on the page's bytes,
         * its geometry from the tables' average entry size */
        const uint64_t avg = D.total ? resident / D.total : 0;
        launch_copy(s, d_oidx, d_smap, rd->d_scanwin, &rd->d_scantot->st,
                    avg ? (cap + avg - 1) / avg : 0, cap, rd->d_page);
    }
    HIP_CHECK(hipEventRecord(rd->ev[3], s));
    HIP_CHECK(hipMemcpyAsync(rd->h_scantot, rd->d_scantot,
                             sizeof(ScanPageTotals), hipMemcpyDeviceToHost,
                             s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    const uint64_t taken = rd->h_scantot->st.n_surv;
    const uint64_t bytes = rd->h_scantot->st.total_out;
    const uint64_t next = rd->h_scantot->next;
    if (taken > max_entries || bytes > cap || next > m) {
        set_err("%s: inconsistent page totals", fn);
        return DBEEL_ERR_HIP;
    }
    if (taken == 0 && next < m) {
        /* the first survivor alone exceeds data_cap (index_cap holds at
         * least one record): ItemTooLarge, cursor untouched */
        page->needed = rd->h_scantot->next_full;
        set_err("%s: entry of %llu bytes does not fit the %llu-byte page "
                "buffer", fn, (unsigned long long)page->needed,
                (unsigned long long)data_cap);
        return DBEEL_ERR_ITEM_TOO_LARGE;
    }
    for (int i = 0; i < 3; i++)
        HIP_CHECK(hipEventElapsedTime(&out.ms[i], rd->ev[i], rd->ev[i + 1]));
    out.taken = taken;
    out.bytes = bytes;
    out.next = next;
    out.shadow = shadow;
    out.d_oidx = d_oidx;
    out.d_rido = d_rido;
    sync_on_fail.dismiss();
    return DBEEL_OK;
}

/* The page is done with: the cursor moves and the page record is filled. */
static void scan_commit(dbeel_gpu_reader_scan* sc, const ScanDrawn& dr,
                        float d2h_ms, dbeel_scan_page* page) {
    sc->cursor += dr.next;
    if (dr.shadow) sc->shadowed += sc->rd->h_scantot->shadowed;
    page->data_len = dr.bytes;
    page->n_entries = dr.taken;
    page->candidates = dr.next;
    page->done = sc->cursor == sc->total;
    page->flag_ms = dr.ms[0];
    page->emit_ms = dr.ms[1];
    page->copy_ms = dr.ms[2];
    page->d2h_ms = d2h_ms;
}

extern "C" int dbeel_gpu_reader_scan_next(dbeel_gpu_reader_scan* sc,
                                          uint8_t* data, size_t data_cap,
                                          uint8_t* index, size_t index_cap,
                                          uint32_t* range_ids,
                                          dbeel_scan_page* page) {
    g_err[0] = 0;
    if (page) memset(page, 0, sizeof *page);
    if (!sc || !page) {
        set_err("reader_scan_next: null scan or page");
        return DBEEL_ERR_INVALID_ARG;
    }
    if (!data || !index || data_cap == 0 || index_cap < 16) {
        set_err("reader_scan_next: data and index buffers must be non-null, "
                "data_cap > 0 and index_cap >= 16");
        return DBEEL_ERR_INVALID_ARG;
    }
    dbeel_gpu_reader* rd = sc->rd;
    if (!sc->snapshot && sc->generation != rd->generation) {
        set_err("reader_scan_next: stale scan (the table list changed since "
                "scan_begin; start a new scan)");
        return DBEEL_ERR_INVALID_ARG;
    }
    ScanDrawn dr;
    int rc = scan_draw("reader_scan_next", sc, data_cap, index_cap, page, dr);
    if (rc || dr.done) return rc;
    hipStream_t s = rd->stream;
    /* on failure nothing of this page may still be in flight into the
     * caller's buffers */
    ScopeGuard sync_on_fail([&] { (void)hipStreamSynchronize(s); });
    HIP_CHECK(hipEventRecord(rd->ev[4], s));
    if (dr.taken) {
        HIP_CHECK(hipMemcpyAsync(data, rd->d_page, dr.bytes,
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(index, dr.d_oidx, dr.taken * 16,
                                 hipMemcpyDeviceToHost, s));
        if (sc->n_ranges && range_ids)
            HIP_CHECK(hipMemcpyAsync(range_ids, dr.d_rido, dr.taken * 4,
                                     hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipEventRecord(rd->ev[5], s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    float d2h = 0;
    HIP_CHECK(hipEventElapsedTime(&d2h, rd->ev[4], rd->ev[5]));
    scan_commit(sc, dr, d2h, page);
    sync_on_fail.dismiss();
    return DBEEL_OK;
}

extern "C" int dbeel_gpu_reader_scan_apply(
    dbeel_gpu_reader_scan* sc, const dbeel_apply_action* actions,
    size_t n_actions, const uint8_t* delete_ts, uint64_t page_bytes,
    uint64_t page_entries, dbeel_scan_page* page,
    dbeel_scan_apply_stats* stats) {
    g_err[0] = 0;
    if (page) memset(page, 0, sizeof *page);
    if (stats) memset(stats, 0, sizeof *stats);
    const char* who = "reader_scan_apply";
    if (!sc || !page) {
        set_err("%s: null scan or page", who);
        return DBEEL_ERR_INVALID_ARG;
    }
    if (!actions) {
        set_err("%s: null actions", who);
        return DBEEL_ERR_INVALID_ARG;
    }
    dbeel_gpu_reader* rd = sc->rd;
    const size_t want = sc->n_ranges ? sc->n_ranges : 1;
    if (n_actions != want) {
        set_err("%s: %zu actions for a scan of %u hash ranges (%zu needed)",
                who, n_actions, sc->n_ranges, want);
        return DBEEL_ERR_INVALID_ARG;
    }
    bool deletes = false;
    for (size_t i = 0; i < n_actions; i++) {
        const int k = actions[i].kind;
        if (k != DBEEL_APPLY_SKIP && k != DBEEL_APPLY_PUT &&
            k != DBEEL_APPLY_DELETE) {
            set_err("%s: action %zu has unknown kind %d", who, i, k);
            return DBEEL_ERR_INVALID_ARG;
        }
        deletes |= k == DBEEL_APPLY_DELETE;
    }
    for (size_t i = 0; i < n_actions; i++)
        if (actions[i].kind != DBEEL_APPLY_SKIP && !actions[i].dst) {
            set_err("%s: action %zu has no destination reader", who, i);
            return DBEEL_ERR_INVALID_ARG;
        }
    for (size_t i = 0; i < n_actions; i++)
        if (actions[i].kind != DBEEL_APPLY_SKIP &&
            actions[i].dst->device != rd->device) {
            set_err("%s: action %zu's destination is on device %d, the scan "
                    "on device %d", who, i, actions[i].dst->device,
                    rd->device);
            return DBEEL_ERR_INVALID_ARG;
        }
    if (deletes && !delete_ts) {
        set_err("%s: a DELETE action needs delete_ts", who);
        return DBEEL_ERR_INVALID_ARG;
    }
    if (page_bytes == 0 || page_entries == 0) {
        set_err("%s: page_bytes and page_entries must be > 0", who);
        return DBEEL_ERR_INVALID_ARG;
    }
    if (!sc->snapshot && sc->generation != rd->generation) {
        set_err("%s: stale scan (the table list changed since scan_begin; "
                "start a new scan)", who);
        return DBEEL_ERR_INVALID_ARG;
    }
    /* a page is one put: fewer than 2^31 entries */
    if (page_entries > 0x7FFFFFFFull) page_entries = 0x7FFFFFFFull;

    /* the groups: distinct (kind, dst) in order of their first range id */
    struct Group {
        int kind;
        dbeel_gpu_reader* dst;
        std::vector<uint8_t> take;
    };
    std::vector<Group> groups;
    for (size_t i = 0; i < n_actions; i++) {
        if (actions[i].kind == DBEEL_APPLY_SKIP) continue;
        Group* g = nullptr;
        for (Group& h : groups)
            if (h.kind == actions[i].kind && h.dst == actions[i].dst) g = &h;
        if (!g) {
            groups.push_back(Group{actions[i].kind, actions[i].dst,
                                   std::vector<uint8_t>(n_actions, 0)});
            g = &groups.back();
        }
        g->take[i] = 1;
    }

    /* the page, finished on the scan reader's stream and left on the
     * device; scan_draw returns with that stream idle */
    ScanDrawn dr;
    int rc = scan_draw(who, sc, page_bytes, page_entries * 16, page, dr);
    if (rc || dr.done) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t n_put = 0, n_del = 0, n_groups = 0;
    if (dr.taken) {
        const PageIn pg = {rd->d_page, dr.bytes, dr.d_oidx, dr.taken,
                           sc->n_ranges ? dr.d_rido : nullptr, true};
        for (Group& g : groups) {
            rc = put_entries_count_check(who, g.dst->mem.count, dr.taken);
            if (rc) return rc;
            dbeel_put_entries_stats st;
            memset(&st, 0, sizeof st);
            /* returns with the destination's stream idle: the next page
             * overwrites a buffer nobody reads */
            rc = put_entries_impl(who, g.dst, pg, g.take.data(),
                                  (uint32_t)n_actions, g.kind, delete_ts,
                                  &st);
            if (rc) return rc; /* earlier groups stay applied, cursor stays */
            (g.kind == DBEEL_APPLY_PUT ? n_put : n_del) += st.selected;
            n_groups++;
        }
    }
    scan_commit(sc, dr, 0.0f, page);
    if (stats) {
        stats->apply_ms = std::chrono::duration<double, std::milli>(
                              std::chrono::steady_clock::now() - t0).count();
        stats->put_entries = n_put;
        stats->delete_entries = n_del;
        stats->skipped = dr.taken - n_put - n_del;
        stats->groups = n_groups;
    }
    return DBEEL_OK;
}

extern "C" int dbeel_gpu_compact_timed(const dbeel_run_view* runs,
                                       size_t n_runs, int keep_tombstones,
                                       int device, dbeel_compact_result* out,
                                       dbeel_compact_timings* t) {
    if (!out) {
        set_err("out is null");
        return DBEEL_ERR_INVALID_ARG;
    }
    dbeel_gpu_job* job = nullptr;
    int rc = dbeel_gpu_job_create(runs, n_runs, device, &job);
    if (rc) return rc;
    rc = dbeel_gpu_job_run(job, keep_tombstones, nullptr, nullptr, t);
    if (!rc) rc = dbeel_gpu_job_fetch(job, out);
    dbeel_gpu_job_destroy(job);
    return rc;
}

extern "C" int dbeel_gpu_compact(const dbeel_run_view* runs, size_t n_runs,
                                 int keep_tombstones, int device,
                                 dbeel_compact_result* out) {
    return dbeel_gpu_compact_timed(runs, n_runs, keep_tombstones, device, out,
                                   nullptr);
}

/* ------------------------------------------------------------------ */
/* Sliced compaction: jobs whose inputs exceed HBM                    */
/*                                                                    */
/* The key space is cut at pivot keys into slices whose input fits    */
/* the device budget; each slice is an ordinary compaction job and    */
/* the outputs concatenate. Because slice boundaries are strict key   */
/* pivots, an equal-key group never splits, so winner/tombstone       */
/* decisions are slice-local and the concatenation is byte-identical  */
/* to one whole compaction (survivors verbatim in global key order,   */
/* offsets rebased). Requires densely-ordered runs (EntryWriter       */
/* layout — verified on-device).                                      */
/* ------------------------------------------------------------------ */

static int host_key_cmp(const uint8_t* a, uint64_t la, const uint8_t* b,
                        uint64_t lb) {
    uint64_t n = la < lb ? la : lb;
    int c = memcmp(a, b, n);
    if (c) return c;
    return la < lb ? -1 : (la > lb ? 1 : 0);
}

/* key view of entry i of a host run; NULL when the index record points
 * outside the run's data (corrupt input must not cause host OOB reads
 * during pivot selection — the device validation would catch it later,
 * but the slicer reads keys FIRST) */
static inline const uint8_t* host_entry_key(const dbeel_run_view* run,
                                            uint64_t i, uint64_t* klen) {
    const uint8_t* rec = run->index + i * 16;
    uint64_t off = ld_u64_host(rec);
    uint32_t key_size, full_size;
    memcpy(&key_size, rec + 8, 4);
    memcpy(&full_size, rec + 12, 4);
    if (key_size < 8 || full_size < 32 ||
        (uint64_t)key_size + 24 > full_size ||
        off > run->data_len || full_size > run->data_len - off)
        return NULL; /* load_entry's test, equally wrap-proof */
    *klen = key_size - 8;
    return run->data + off + 8;
}

/* Bytes of a compaction's input (what the slice count is sized from), with
 * the run that has the most entries (where the pivots come from) and its
 * entry count. */
static uint64_t input_extent(const dbeel_run_view* runs, size_t n_runs,
                             size_t* big_run, uint64_t* max_count) {
    uint64_t total_input = 0;
    *big_run = 0;
    *max_count = 0;
    for (size_t r = 0; r < n_runs; r++) {
        total_input += runs[r].data_len + runs[r].index_len;
        uint64_t c = runs[r].index_len / 16;
        if (c > *max_count) {
            *max_count = c;
            *big_run = r;
        }
    }
    return total_input;
}

/* The host slicer: S slices of every run. Pivots are evenly spaced keys of
 * the largest run, bounds[r][sl] the first entry of run r not below pivot sl
 * (S + 1 values, from 0 to the run's count, appended to the n_runs empty
 * lists the caller passes). cut[r][sl] is the data offset where slice sl of
 * run r begins, read from the record AT the boundary; every record read here
 * passes host_entry_key's bounds test first. */
static int slice_runs(const dbeel_run_view* runs, size_t n_runs,
                      size_t big_run, uint64_t max_count, uint64_t S,
                      std::vector<std::vector<uint64_t>>& bounds,
                      std::vector<std::vector<uint64_t>>& cut) {
    std::vector<std::pair<const uint8_t*, uint64_t>> pivots; /* key,len */
    for (uint64_t j = 1; j < S; j++) {
        uint64_t klen;
        const uint8_t* k =
            host_entry_key(&runs[big_run], j * max_count / S, &klen);
        if (!k) {
            set_err("corrupt index record in run %zu", big_run);
            return DBEEL_ERR_CORRUPT;
        }
        pivots.push_back({k, klen});
    }
    for (size_t r = 0; r < n_runs; r++) {
        const uint64_t n = runs[r].index_len / 16;
        bounds[r].push_back(0);
        cut[r].push_back(0);
        for (auto& pv : pivots) {
            uint64_t lo = bounds[r].back(), hi = n;
            while (lo < hi) {
                uint64_t mid = (lo + hi) >> 1;
                uint64_t kl;
                const uint8_t* k = host_entry_key(&runs[r], mid, &kl);
                if (!k) {
                    set_err("corrupt index record in run %zu", r);
                    return DBEEL_ERR_CORRUPT;
                }
                if (host_key_cmp(k, kl, pv.first, pv.second) < 0)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            uint64_t c = runs[r].data_len;
            if (lo == 0) {
                c = 0;
            } else if (lo < n) {
                uint64_t kl;
                if (!host_entry_key(&runs[r], lo, &kl)) {
                    set_err("corrupt index record in run %zu", r);
                    return DBEEL_ERR_CORRUPT;
                }
                c = ld_u64_host(runs[r].index + lo * 16);
            }
            if (c < cut[r].back()) {
                set_err("run %zu: index offsets not ascending", r);
                return DBEEL_ERR_CORRUPT;
            }
            bounds[r].push_back(lo);
            cut[r].push_back(c);
        }
        bounds[r].push_back(n);
        cut[r].push_back(runs[r].data_len);
    }
    return DBEEL_OK;
}

extern "C" int dbeel_gpu_compact_sliced(const dbeel_run_view* runs,
                                        size_t n_runs, int keep_tombstones,
                                        int device,
                                        uint64_t max_resident_bytes,
                                        dbeel_compact_result* out) {
    g_err[0] = 0;
    if (!out) {
        set_err("out is null");
        return DBEEL_ERR_INVALID_ARG;
    }
    int rc = validate_runs(runs, n_runs);
    if (rc) return rc;
    rc = check_device_arg(device);
    if (rc) return rc;
    size_t big_run;
    uint64_t max_count;
    const uint64_t total_input =
        input_extent(runs, n_runs, &big_run, &max_count);
    uint64_t budget = max_resident_bytes;
    if (!budget) {
        HIP_CHECK(hipSetDevice(device));
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        /* input slab + output data + pfx/aux/cr/rrec intermediates stay
         * under ~2.6x input for <= 64 runs; /3 leaves headroom */
        budget = (uint64_t)(free_b / 3);
    }
    uint64_t S = budget ? (total_input + budget - 1) / budget : 1;
    if (S <= 1 || max_count < 2 * S)
        return dbeel_gpu_compact(runs, n_runs, keep_tombstones, device, out);

    /* the slice views take their data offsets from the index records
     * themselves (off_lo / off_hi below): cut is not needed here */
    std::vector<std::vector<uint64_t>> bounds(n_runs), cut(n_runs);
    rc = slice_runs(runs, n_runs, big_run, max_count, S, bounds, cut);
    if (rc) return rc;

    memset(out, 0, sizeof *out);
    std::vector<uint8_t> acc_data, acc_index;
    uint64_t written = 0;
    std::vector<uint8_t> idx_tmp;
    for (uint64_t sl = 0; sl < S; sl++) {
        std::vector<dbeel_run_view> views;
        std::vector<size_t> idx_tmp_off;
        idx_tmp.clear();
        uint64_t slice_entries = 0;
        for (size_t r = 0; r < n_runs; r++) {
            uint64_t lo = bounds[r][sl], hi = bounds[r][sl + 1];
            dbeel_run_view v{};
            if (hi > lo) {
                uint64_t off_lo = ld_u64_host(runs[r].index + lo * 16);
                uint64_t off_hi =
                    (hi < runs[r].index_len / 16)
                        ? ld_u64_host(runs[r].index + hi * 16)
                        : runs[r].data_len;
                v.data = runs[r].data + off_lo;
                v.data_len = off_hi - off_lo;
                /* rebased index records */
                size_t pos = idx_tmp.size();
                idx_tmp.resize(pos + (hi - lo) * 16);
                memcpy(idx_tmp.data() + pos, runs[r].index + lo * 16,
                       (hi - lo) * 16);
                for (uint64_t i = 0; i < hi - lo; i++) {
                    uint64_t o =
                        ld_u64_host(idx_tmp.data() + pos + i * 16) - off_lo;
                    memcpy(idx_tmp.data() + pos + i * 16, &o, 8);
                }
                idx_tmp_off.push_back(pos);
                v.index_len = (hi - lo) * 16;
                slice_entries += hi - lo;
            } else {
                v.data = runs[r].data; /* non-null, zero-length */
                v.data_len = 0;
                v.index = runs[r].index;
                v.index_len = 0;
                idx_tmp_off.push_back((size_t)-1);
            }
            views.push_back(v);
        }
        if (!slice_entries) continue;
        /* resolve idx pointers after idx_tmp stopped growing */
        for (size_t r = 0; r < n_runs; r++)
            if (idx_tmp_off[r] != (size_t)-1)
                views[r].index = idx_tmp.data() + idx_tmp_off[r];
        dbeel_compact_result sres{};
        rc = dbeel_gpu_compact(views.data(), n_runs, keep_tombstones,
                               device, &sres);
        if (rc) return rc;
        /* concatenate, rebasing index offsets */
        uint64_t base = acc_data.size();
        acc_data.insert(acc_data.end(), sres.data,
                        sres.data + sres.data_len);
        size_t ipos = acc_index.size();
        acc_index.insert(acc_index.end(), sres.index,
                         sres.index + sres.index_len);
        for (uint64_t i = 0; i < sres.index_len / 16; i++) {
            uint64_t o =
                ld_u64_host(acc_index.data() + ipos + i * 16) + base;
            memcpy(acc_index.data() + ipos + i * 16, &o, 8);
        }
        written += sres.entries_written;
        dbeel_gpu_result_free(&sres);
    }

    out->data = (uint8_t*)malloc(acc_data.size() ? acc_data.size() : 1);
    out->index = (uint8_t*)malloc(acc_index.size() ? acc_index.size() : 1);
    if (!out->data || !out->index) {
        free(out->data);
        free(out->index);
        memset(out, 0, sizeof *out);
        set_err("host alloc failed");
        return DBEEL_ERR_OOM;
    }
    memcpy(out->data, acc_data.data(), acc_data.size());
    memcpy(out->index, acc_index.data(), acc_index.size());
    out->data_len = acc_data.size();
    out->index_len = acc_index.size();
    out->entries_written = written;
    return DBEEL_OK;
}

/* ------------------------------------------------------------------ */
/* Compaction into caller buffers: slices pipelined, filter across     */
/* slices. See include/dbeel_gpu.h.                                    */
/* ------------------------------------------------------------------ */

/* Grows the call's hash array to `need` bytes keeping its first `used`
 * bytes; the copy and the free are ordered on s. */
static int hashes_reserve(ulonglong2** p, uint64_t* cap, uint64_t used,
                          uint64_t need, hipStream_t s) {
    if (need <= *cap) return DBEEL_OK;
    uint64_t want = need + need / 4;
    ulonglong2* np = nullptr;
    HIP_CHECK(hipMalloc(&np, want));
    if (used) {
        hipError_t e = hipMemcpyAsync(np, *p, used, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipFree(np);
            HIP_CHECK(e);
        }
    }
    (void)hipFree(*p);
    *p = np;
    *cap = want;
    return DBEEL_OK;
}

extern "C" int dbeel_gpu_compact_into(
    const dbeel_run_view* runs, size_t n_runs, int keep_tombstones,
    int device, uint64_t max_resident_bytes, uint32_t n_slices, uint8_t* data,
    uint64_t data_cap, uint8_t* index, uint64_t index_cap, int want_bloom,
    uint8_t** bloom_bytes, uint64_t* bloom_len,
    dbeel_compact_into_result* result, dbeel_compact_into_stats* stats) {
    g_err[0] = 0;
    const auto t_begin = std::chrono::steady_clock::now();
    if (!result) {
        set_err("compact_into: result is null");
        return DBEEL_ERR_INVALID_ARG;
    }
    memset(result, 0, sizeof *result);
    if (stats) memset(stats, 0, sizeof *stats);
    if (bloom_bytes) *bloom_bytes = nullptr;
    if (bloom_len) *bloom_len = 0;
    if (!data || !index) {
        set_err("compact_into: data or index is null");
        return DBEEL_ERR_INVALID_ARG;
    }
    if (want_bloom && (!bloom_bytes || !bloom_len)) {
        set_err("compact_into: want_bloom needs bloom_bytes and bloom_len");
        return DBEEL_ERR_INVALID_ARG;
    }
    if (!runs || n_runs == 0 || n_runs > MAX_RUNS) {
        set_err("compact_into: runs is null, empty or more than %d", MAX_RUNS);
        return DBEEL_ERR_INVALID_ARG;
    }
    int rc = check_device_arg(device);
    if (rc) return rc;
    rc = validate_runs(runs, n_runs);
    if (rc) return rc;

    size_t big_run;
    uint64_t max_count;
    const uint64_t total_input =
        input_extent(runs, n_runs, &big_run, &max_count);
    uint64_t S = n_slices;
    if (!S) {
        uint64_t budget = max_resident_bytes;
        if (!budget) {
            rc = select_device(device);
            if (rc) return rc;
            size_t free_b = 0, total_b = 0;
            HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            /* compact_sliced keeps one job under a third of free memory
             * (~2.6x input per job); two jobs are alive here */
            budget = (uint64_t)(free_b / 6);
        }
        S = budget ? (total_input + budget - 1) / budget : 1;
    }
    if (S > max_count / 2) S = max_count / 2;
    if (S < 1) S = 1;

    std::vector<std::vector<uint64_t>> bounds(n_runs), cut(n_runs);
    rc = slice_runs(runs, n_runs, big_run, max_count, S, bounds, cut);
    if (rc) return rc;

    rc = select_device(device);
    if (rc) return rc;

    dbeel_gpu_job* prev = nullptr; /* its fetch may be in flight */
    bool prev_fetching = false;
    hipEvent_t f0 = nullptr, f1 = nullptr;
    hipStream_t bs = nullptr;      /* the call's own: the filter's fill */
    ulonglong2* d_hashes = nullptr;
    uint64_t hashes_cap = 0;
    uint32_t* d_bits = nullptr;
    ScopeGuard cleanup([&] {
        if (prev) {
            (void)hipStreamSynchronize(prev->stream);
            dbeel_gpu_job_destroy(prev);
        }
        (void)hipFree(d_hashes);
        (void)hipFree(d_bits);
        if (f0) (void)hipEventDestroy(f0);
        if (f1) (void)hipEventDestroy(f1);
        if (bs) (void)hipStreamDestroy(bs);
    });
    HIP_CHECK(hipEventCreate(&f0));
    HIP_CHECK(hipEventCreate(&f1));

    dbeel_compact_into_stats st{};
    uint64_t off_d = 0, off_i = 0, entries = 0;
    bool short_caps = false;
    float up_a = 0, up_b = 0; /* next upload's span, ms after prev's f0 */
    bool up_valid = false;

    /* waits for prev's copies, books their time and overlap, destroys it */
    auto retire_prev = [&]() -> int {
        if (!prev) return DBEEL_OK;
        dbeel_gpu_job* j = prev;
        prev = nullptr;
        ScopeGuard drop([&] { dbeel_gpu_job_destroy(j); });
        HIP_CHECK(hipStreamSynchronize(j->stream));
        HIP_CHECK(hipGetLastError());
        if (prev_fetching) {
            float f = 0;
            HIP_CHECK(hipEventElapsedTime(&f, f0, f1));
            st.d2h_ms += f;
            if (up_valid) {
                float lo = up_a > 0 ? up_a : 0, hi = up_b < f ? up_b : f;
                if (hi > lo) st.overlap_ms += hi - lo;
            }
        }
        prev_fetching = false;
        up_valid = false;
        return DBEEL_OK;
    };

    std::vector<dbeel_run_view> views(n_runs);
    std::vector<uint64_t> bias(n_runs);
    const uint32_t one[1] = {(uint32_t)n_runs};
    for (uint64_t sl = 0; sl < S; sl++) {
        uint64_t slice_entries = 0, slice_bytes = 0;
        for (size_t r = 0; r < n_runs; r++) {
            const uint64_t lo = bounds[r][sl], hi = bounds[r][sl + 1];
            const uint64_t c0 = cut[r][sl], c1 = cut[r][sl + 1];
            /* an empty view keeps non-null pointers, as compact_sliced's */
            views[r] = {runs[r].data + c0, hi > lo ? c1 - c0 : 0,
                        runs[r].index + lo * 16, (hi - lo) * 16};
            bias[r] = hi > lo ? c0 : 0;
            slice_entries += hi - lo;
            slice_bytes += views[r].data_len + views[r].index_len;
        }
        if (!slice_entries) continue;

        dbeel_gpu_job* job = nullptr;
        rc = job_create_impl(views.data(), n_runs, one, 1, device, &job,
                             false, bias.data());
        if (rc) return rc;
        ScopeGuard drop_job([&] { dbeel_gpu_job_destroy(job); });
        st.slices++;
        st.bytes_in += slice_bytes;
        st.h2d_ms += job->h2d_ms;
        if (prev_fetching) {
            /* job_create has waited for its own stream only: prev's copies
             * went on meanwhile. ev[0] / ev[1] still bracket the upload. */
            up_valid =
                hipEventElapsedTime(&up_a, f0, job->ev[0]) == hipSuccess &&
                hipEventElapsedTime(&up_b, f0, job->ev[1]) == hipSuccess;
            (void)hipGetLastError();
        }
        uint64_t dl = 0, ne = 0;
        dbeel_compact_timings tm{};
        rc = dbeel_gpu_job_run(job, keep_tombstones, &dl, &ne, &tm);
        if (rc) return rc;
        st.kernel_ms += tm.kernel_ms;

        /* the one wait per slice: after it no earlier job's stream holds
         * work, so the hash array may move and the events may be reused */
        rc = retire_prev();
        if (rc) return rc;
        if (off_d + dl > data_cap || off_i + ne * 16 > index_cap)
            short_caps = true;
        if (want_bloom && !short_caps && ne) {
            rc = hashes_reserve(&d_hashes, &hashes_cap, entries * 16,
                                (entries + ne) * 16, job->stream);
            if (rc) return rc;
            hipLaunchKernelGGL(k_bloom_hash, dim3(pick_grid(ne, 256)),
                               dim3(256), 0, job->stream, job->d_outdata,
                               job->d_outindex, ne, (uint64_t)BLOOM_SEED,
                               d_hashes + entries);
        }
        if (!short_caps && ne) {
            rc = job_fetch_into_async(job, data + off_d, index + off_i, off_d,
                                      f0, f1);
            if (rc) {
                (void)hipStreamSynchronize(job->stream);
                return rc;
            }
            prev_fetching = true;
        }
        off_d += dl;
        off_i += ne * 16;
        entries += ne;
        drop_job.dismiss();
        prev = job;
    }
    rc = retire_prev();
    if (rc) return rc;

    result->data_len = off_d;
    result->index_len = off_i;
    result->entries_written = entries;
    st.bytes_out = off_d + off_i;
    auto finish_stats = [&] {
        st.wall_ms = std::chrono::duration<double, std::milli>(
                         std::chrono::steady_clock::now() - t_begin).count();
        if (stats) *stats = st;
    };
    if (short_caps) {
        finish_stats();
        set_err("compact_into: output needs %llu data and %llu index bytes, "
                "caps are %llu and %llu", (unsigned long long)off_d,
                (unsigned long long)off_i, (unsigned long long)data_cap,
                (unsigned long long)index_cap);
        return DBEEL_ERR_ITEM_TOO_LARGE;
    }
    if (want_bloom) {
        /* every job's stream has been waited for: the hashes are complete */
        const uint64_t n_bits = bloom_bits_for(entries);
        const uint64_t n_words = (n_bits + 31) / 32;
        HIP_CHECK(hipStreamCreate(&bs));
        HIP_CHECK(hipMalloc(&d_bits, n_words * 4));
        HIP_CHECK(hipMemsetAsync(d_bits, 0, n_words * 4, bs));
        if (entries)
            hipLaunchKernelGGL(k_bloom_fill, dim3(pick_grid(entries, 256)),
                               dim3(256), 0, bs, d_hashes, entries, n_bits,
                               BLOOM_K, d_bits);
        ReaderTable t;
        t.d_bits = (uint8_t*)d_bits;
        t.bloom = {t.d_bits, n_bits, BLOOM_SEED, BLOOM_K, 0};
        rc = table_bloom_fetch(t, bs, bloom_bytes, bloom_len);
        if (rc) return rc;
        HIP_CHECK(hipGetLastError());
    }
    finish_stats();
    return DBEEL_OK;
}

extern "C" void dbeel_gpu_result_free(dbeel_compact_result* r) {
    if (!r) return;
    free(r->data);
    free(r->index);
    memset(r, 0, sizeof *r);
}
