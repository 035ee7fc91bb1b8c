/*
 * csvplus_hip.h — C ABI of libcsvplus_hip: the MI355X (gfx950) implementation
 * of csvplus's Index-build + Join hot path.
 *
 * The reference (maxim2266/csvplus, one Go file) has no FFI layer; the seams a
 * cgo shim replaces are (all citations are file:line in the reference):
 *
 *   sort.Sort(&index.impl)                      csvplus.go:736   -> cph_index_build
 *   createUniqueIndex adjacent-equal scan       csvplus.go:749-753 -> cph_index_build(unique=1)
 *   Join per-row  first() + forward scan        csvplus.go:557-563 -> cph_join_probe
 *   Except per-row has()                        csvplus.go:599-602 -> cph_join_probe (cnt==0 rows)
 *   indexImpl.find (Find / SubIndex bounds)     csvplus.go:870-891 -> cph_index_find
 *
 * Conventions
 *   - Every function returns an int32 status (CPH_OK == 0, errors < 0) unless
 *     noted.  cph_last_error(ctx) gives a NUL-terminated message owned by the
 *     ctx, valid until the next call on that ctx.
 *   - Inputs are borrowed for the duration of the call only.  Outputs
 *     (cph_index, cph_matches) are library-owned and explicitly released.
 *   - A cph_ctx is single-threaded (the reference has no concurrency either:
 *     no go/sync/chan in csvplus.go).  The library calls hipSetDevice on every
 *     entry, so a ctx may migrate between OS threads (cgo does that).
 *   - No callbacks into the caller.  No exceptions cross the boundary.
 *   - String columns are Arrow-style: `data` holds the concatenated raw value
 *     bytes (no terminators, any byte value incl. NUL), `offsets` has
 *     nrows+1 monotonically non-decreasing entries of 32 or 64 bits.
 *     `mem` says where both arrays live: host memory (pageable or pinned) or
 *     device memory of the ctx's GPU.
 *   - Row ids are uint32: a single table is limited to 2^32-1 rows
 *     (CPH_ERR_TOO_MANY_ROWS otherwise).  Go `int` row counts are 64-bit; the
 *     shim must check.
 *
 * Ordering contract (csvplus.go:794-807, indexImpl.Less): rows are ordered by
 * the tuple of key columns, each compared with strings.Compare = unsigned
 * bytewise lexicographic, a proper prefix sorting first.  Rows with equal keys
 * keep their input order (stable), which is one of the orders the reference's
 * unstable sort.Sort may produce (parity class P1).
 */
#ifndef CSVPLUS_HIP_H
#define CSVPLUS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPH_API __attribute__((visibility("default")))

/* ---- status codes ---------------------------------------------------------- */
enum {
    CPH_OK                 = 0,
    CPH_ERR_INVALID        = -1,  /* bad argument (NULL, nkeycols<=0, offset_bits...)        */
    CPH_ERR_HIP            = -2,  /* a HIP runtime call failed; see cph_last_error           */
    CPH_ERR_NO_DEVICE      = -3,  /* no usable GPU: the library never falls back to the CPU  */
    CPH_ERR_DUPLICATE      = -4,  /* unique index requested and equal keys exist             */
    CPH_ERR_TOO_MANY_ROWS  = -5,  /* nrows > 2^32-1                                          */
    /* -6 is retired: key length is unlimited (keys beyond 128 byte positions are cut into codec windows) */
    CPH_ERR_TOO_MANY_COLS  = -7,  /* join with more columns than the index has
                                     (csvplus.go:548-550 panics "too many source columns")   */
    CPH_ERR_NOMEM          = -8
};

#define CPH_MAX_KEY_COLS  16

enum { CPH_MEM_HOST = 0, CPH_MEM_DEVICE = 1 };

typedef struct cph_ctx   cph_ctx;
typedef struct cph_index cph_index;

/* One string column (or a row range of one). */
typedef struct {
    const uint8_t* data;        /* concatenated value bytes                               */
    const void*    offsets;     /* nrows+1 entries; value i = data[offsets[i]..offsets[i+1]) */
    uint64_t       nrows;
    int32_t        offset_bits; /* 32 or 64                                               */
    int32_t        mem;         /* CPH_MEM_HOST or CPH_MEM_DEVICE                         */
    uint32_t       fixed_width; /* > 0: every value has exactly this many bytes, value i =
                                   data[i*fixed_width ..); offsets is ignored (may be NULL).
                                   Saves the offsets' HBM traffic and a dependent load.   */
    uint32_t       reserved_;
} cph_strcol;

/* One key value (for cph_index_find). Host memory. */
typedef struct {
    const uint8_t* data;
    uint64_t       len;
} cph_strval;

/*
 * Result of a probe.  All arrays live in `mem` (as requested by the caller)
 * and stay valid until cph_matches_release.
 *
 *   lo[i], cnt[i]   for probe row i: the matching index rows are the sorted
 *                   positions [lo[i], lo[i]+cnt[i]).  cnt==0 means no match
 *                   (lo is then unspecified) — the reference's
 *                   `for i := first(values); i<n && !cmp(i,values,false); i++`
 *                   (csvplus.go:559) runs cnt[i] times.
 *   probe_idx[m], build_row[m]   m < nmatches: the joined pairs in the
 *                   reference's emission order (stream order, then ascending
 *                   index position, csvplus.go:553-567).  probe_idx is
 *                   probe_base + the row's position in this call; build_row is
 *                   the ORIGINAL row id of the index row (its position in the
 *                   table handed to cph_index_build), i.e. perm[lo+j].
 */
typedef struct {
    uint64_t        nprobe;
    uint64_t        nmatches;
    const uint32_t* lo;
    const uint32_t* cnt;
    const uint64_t* probe_idx;
    const uint32_t* build_row;
    int32_t         mem;
    int32_t         reserved_;
} cph_matches;

/* ---- context --------------------------------------------------------------- */

/* Creates a context bound to HIP device `device_id`.  Fails with
 * CPH_ERR_NO_DEVICE when the device does not exist (there is no CPU path). */
CPH_API int32_t cph_ctx_create(int32_t device_id, cph_ctx** out);
CPH_API void    cph_ctx_destroy(cph_ctx* ctx);
CPH_API const char* cph_last_error(const cph_ctx* ctx);

/* All work of this ctx is enqueued on `hip_stream` (a hipStream_t; NULL = the
 * ctx's own stream).  Lets a host framework (torch, a Go scheduler) order the
 * library's kernels with its own copies. */
CPH_API int32_t cph_ctx_set_stream(cph_ctx* ctx, void* hip_stream);

/* Measurement / tuning knobs (tools/microbench), per ctx — two devices in one process never share them:
 *   "chain_debug"   attribution switches of the chained-join kernel: bit 0 skips the table lookups, bit 1 the
 *                   key encode, bit 2 the result stores.  Results are WRONG while any bit is set; 0 = product path.
 *   "sort_threads"  256 / 512: workgroup size of the radix sort (0 = automatic)
 *   "sort_rbits"    8 / 9: digit width of the radix sort (0 = automatic)
 *   "sort_xcd_tiles" 0 / 1: the scatter kernel gives every XCD a contiguous range of tiles (default 1)
 *   "sort_digit_stream" 0 / 1 (default 1): a radix scatter over 64-bit keys leaves the next pass's digits behind as a byte stream, so that
 *                   pass's histogram reads 1 byte per key instead of 8
 *   "chain_nt_streams" 0 / 1 / 2 (default 0): the chained Join loads the stream's bytes and stores its results non-temporally — never,
 *                   always, in positions mode only (measured: within 1 %)
 *   "speculative_groups"  dictionary windows of long keys on large inputs: 0 = always the exact pass over all rows,
 *                   1 = dictionaries straight from the row sample when every value of every chosen window is COMMON in it
 *                   (met 16 times or more: a closed vocabulary; default),
 *                   2 = always from the sample (the encode kernel completes them; a test hook)
 *   "plan_threads" / "gstats_threads"  workgroup sizes of the dictionary encode / window statistics kernels (0 = default)
 *   "join_hash"     0: indexes built on this ctx never get a hash table — their sparse-key Joins binary-search the
 *                   sorted codes as before (A/B switch for measurements and for the fallback's tests; default 1)
 *   "codec_split"   0 / 1 (default 1): keys that do not code in 32 bits are tried with the delimiter split — the costliest
 *                   variable-length key column cut at its first delimiter byte into a dictionary-coded prefix and a
 *                   per-position suffix (floating fields like "Smith/Amelia#12345": 25 bits instead of 47; A/B switch)
 *   "direct_fused_encode" 0 / 1 (default 1): the direct sort of ONE fixed-width 8-byte key column under an arithmetic codec (decimal ids; the
 *                   column 16-byte aligned) codes the keys inside its first partition level — no encode kernel, no 4-byte code per row written
 *                   and read again (1e8 ids: 1.30 -> 1.12 ms; A/B switch)
 *   "direct_ranktab" 0 / 1 (default 1): the window sort of a code space larger than its table writes the Join's rank table (presence bits +
 *                   keys before, 8 bytes per 32 codes) while it streams its windows out: a Join that reports positions finds it ready
 *                   (0: built by the first such Join, k_build_ranktab; A/B switch)
 *   "chain_prejoin" 0 / 1 (default 1): chain steps whose key is a column of an earlier step's build table (cph_chain_step.source != 0)
 *                   are answered from PRE-JOINED tables when the stream is at least twice as long as those tables: the build sides are
 *                   joined with each other first (one pass over the table's column), the stream rows then need one 4-byte gather per
 *                   such step (0: the fused kernel gathers and encodes the key per stream row; A/B switch)
 *   "hash_load_pct" 25..90 (default 50): load factor of the Join hash tables (sparse key spaces), per cent of a 64-byte sector's slots,
 *                   counted in DISTINCT keys (rounds 3-4 counted rows).  Measured at 1e7 keys x 1e8 probes: 50 % 2.69 ms, 75 % 3.58 ms,
 *                   85 % 5.5 ms — a smaller table does not pay for the longer probe sequences (profiles/r05_tried_not_kept.txt)
 *   "split_speculative" 0 / 1 (default 1): IndexOn over ONE variable-length key column of >= 2^22 rows takes the split codec's prefix
 *                   dictionary and suffix alphabets from its 2^18-row sample alone; the encode kernel checks every row against them
 *                   (prefix in the dictionary, every suffix byte and the end of the suffix in its position's alphabet, lengths within
 *                   the sample's) and a row it cannot code makes the build start over with the exact statistics pass — the index
 *                   is the same either way (A/B switch: 0 = always the exact pass)
 *   "scan_lookback" 0 / 1 (default 1): the 32-bit exclusive scans (radix count matrices, compaction offsets) run as ONE launch
 *                   (decoupled look-back) instead of three (A/B switch)
 *   "counted_sort"  0 / 1 (default 1): IndexOn over one-word 32-bit codes WITH duplicates (>= 2^21 rows) sorts through counted LDS windows
 *                   (rows per window of the code space counted first, two partition levels into exactly sized buckets, every window
 *                   counting-sorted in LDS with equal keys put in row order) instead of 3-4 radix passes; a window beyond 16384 rows
 *                   (one key with more duplicates, a dense cluster in a sparse code space) is noticed on the device and the classic
 *                   passes sort the same codes.  Same index either way (A/B switch)
 *   "csv_fast"      0 / 1 (default 1): cph_csv_parse first tries byte-parallel passes over 16 KiB text tiles (texts without any quote,
 *                   no TrimLeadingSpace, <= 8 columns, < 4 GiB, no blank / comment line inside, records that end within 4 KiB of their
 *                   tile); anything else — and every error — goes through the record-parallel kernels.  Same columns either way
 *   "csv_onepass"   0 / 1 / N (default 1): cph_csv_write[_rows] over >= 4096 rows with at least one such group renders the text in ONE pass: every
 *                   group of adjacent columns gathered from one table (<= the output's rows) through one row-id array is rendered once per
 *                   table row into a slot table ([length][CSV text], stride 16..128 bytes: one aligned fetch per output row and table),
 *                   a tile of 256 / 512 records learns its place in the text from a decoupled look-back over the tiles before it
 *                   (persistent grid, no length array, no scan) and leaves through LDS.  Not taken (-> the two-pass writer, same bytes):
 *                   more than 8 output columns after grouping, a fragment beyond 127 bytes, records beyond ~72 bytes on average, a
 *                   buffer estimate (stream columns' bytes + 1/8 for quotes) that a tile overruns.  0: always the two passes; N > 1: the
 *                   one pass whatever the row count, with at most N workgroups (tests)
 *                   The one-pass kernel is a persistent grid whose tiles wait for the tiles in front of them: the library runs one at a time per
 *                   device and process; two PROCESSES that write CSV on the same GPU at the same moment should set 0
 *   "csv_onepass_debug" bits (default 0; measurement only, the text is wrong when set): 1 = no look-back, 2 = no record bytes, 4 = one
 *                   record per thread
 *   "direct_sort"   0 / 1 (default 1): a build that expects distinct keys (cph_index_build with unique = 1, cph_index_spec.unique) over a
 *                   dense 32-bit code space (rows <= code states <= 2 rows: decimal ids, row numbers) sorts without radix passes: the rows
 *                   are split by the top bits of their codes into 2^14-slot windows, every window is filled in LDS (slot = code) and
 *                   streamed out — all global stores sequential; a duplicate is noticed on the device and the build starts over the
 *                   general way, which also reports where the first duplicate is.  0: always the general way (A/B switch); any other
 *                   value fails with CPH_ERR_INVALID and leaves the setting as it was
 *   "float_device"  0 / 1 (default 0): 1 = every float conversion (cph_col_to_number with CPH_NUM_FLOAT64 and what shares its path: float
 *                   compare terms of cph_filter_rows, float specs of cph_index_aggregate, a float order column of cph_index_resolve, the
 *                   float leaves of cph_num_eval) decides the valid values OUTSIDE Clinger's exact cases on the device as well, with the
 *                   Eisel-Lemire conversion (one or two 64 x 64 -> 128-bit multiplies by a tabulated power of five); only a value that
 *                   routine cannot decide — a few per thousand of those with non-zero digits behind the 19th significant one, none
 *                   of the others — is finished on the host, and `host_rows` of every result counts just those.  0: all values
 *                   outside Clinger's cases are finished on the host, 128 bytes per row over the bus.  Same values, status bytes and
 *                   error report either way; any other value fails with CPH_ERR_INVALID and leaves the setting as it was
 *   "stats_sample"  0 / 1 (default 1): IndexOn over ONE fixed-width key column (<= 40 bytes) of >= 2^20 rows learns its per-position
 *                   alphabets from ~65 536 rows spread over the table instead of a pass over all rows; the encode kernel checks every
 *                   row against them, and a row with a byte the sample did not show makes the build start over with the exact
 *                   pass (the index is the same either way; A/B switch)
 *   "host_build"    0 / 1 (default 1): cph_index_build over ONE key column of at most 8 byte positions (decimal ids, short tags) of
 *                   >= 2^20 rows that lives in HOST memory forms the key codes on the host — alphabets from a sample of the rows,
 *                   the codes by the ctx's worker pool in 2^22-row chunks, each uploaded (4 bytes per row instead of the strings)
 *                   while the next is coded — and the device only sorts; a row the sampled alphabets cannot code, or duplicates under
 *                   the optimistic direct sort, send the build down the general path (upload of the strings).  Same index either way.
 *   "host_threads"  threads of that worker pool (default 0: half the hardware threads, at most 32: the loops are bound by the
 *                   memory bandwidth of the NUMA node that holds the pinned buffers well before that)
 *   "host_split"    0 / 1 / 2 (default 1): the same for ONE variable-length key column of >= 2^22 rows in HOST memory whose values
 *                   want the delimiter split ("Smith/Amelia#12345": a prefix dictionary + suffix positions, 25 bits for BASELINE
 *                   config 3's 10-22 byte keys): the codec comes from the sample the device would take, read by the host's threads,
 *                   the codes (4 bytes per row instead of ~22 bytes of string) from a loop that checks every row like the device's
 *                   encode kernel — unknown prefix, foreign suffix byte, longer value: the strings are uploaded after all.  Same index.
 *                   1: taken when the estimate says the host's threads beat the upload (~20 ns per row and thread against ~50 GB/s of
 *                   PCIe; the threads counted are those the cgroup's CPU QUOTA allows — a container throttled to 16 CPUs codes 1e8
 *                   rows in ~100 ms, the upload takes 44), 2: always, 0: never
 *   "host_split_threads" threads of that loop's own pool (default 0: 3/8 of the hardware threads, at most 96, at most the CPU quota —
 *                   it computes, where the 8-byte loops wait for memory)
 *   "host_numa"     0 / 1 (default 0): 1 binds that pool's workers to the CPUs of the NUMA node that holds the column's first page
 *                   (opt-in: its effect could not be measured on the quota-limited test hosts)
 *   "hash_partitioned" 0 / 1 / 2 (default 1): the hash table of a duplicate-free index of >= 2^21 keys (sparse key codes: random ids,
 *                   hashes) is built SLICE BY SLICE: the rows grouped by the 64 KB slice of the table their home sector lies in, every
 *                   slice filled in LDS by one workgroup and written out once (probe sequences wrap inside a slice) instead of
 *                   compare-and-swaps all over the table; 0: the latter; 2: slice by slice whatever the size (tests).  Lookups answer
 *                   the same either way
 *   "build_side_stream" 0 / 1 (default 1): cph_index_build_many enqueues every second build of a batch on a second stream of
 *                   the ctx, so the launch-latency-bound kernels of a small table run beside its neighbour's instead of behind
 *                   them; both streams are idle when the call returns (A/B switch)
 *   "codec_debug"   1: the window choice of every index build (and the phase times of a one-launch build) go to stderr
 *   "small_build_rows"  tables of at most this many rows (default 8192, at most 16384) are indexed by ONE launch of one
 *                   workgroup and one synchronisation (small_build.hip); 0 = always the general path
 *   "chain_rank_lds"  0 / 1: a Join that reports positions copies the rank tables of small indexes into LDS (default 1)
 *   "chain_rows4"   0 / 1 / 2 (default 1): the register-heavy variants of the fused chained Join (keys beyond 8 bytes with 64-bit codes
 *                   from two steps on, long or wide chains from three steps on) keep 4 rows per lane in flight instead of 8, which
 *                   lets three waves per SIMD run instead of one; 0 = always 8, 2 = every general (non-lean) chain 4 (A/B switch)
 *   "chain_arith"   0 / 1 (default 1): the fused chained Join encodes fixed-width key columns over contiguous alphabets
 *                   (decimal ids) arithmetically — one aligned 8-byte load and a dot product instead of a LUT walk (A/B switch)
 *   "chain_identity" 0 / 1 (default 1): reporting positions, an index whose code space has exactly as many states as the
 *                   index has rows needs no lookup: the position of a key is its code (A/B switch)
 *   "order_select"  0 / 1 / 2 (default 1): cph_order_rows with a limit that is small against the row count radix-selects the rows
 *                   that can reach the result and sorts only those; 0 = always the full sort, 2 = the select for every limit,
 *                   whatever the row count (measuring where the two routes cross; A/B switch: the answer is the same)
 *   "pool_reserve_mb"  reserves ONE device slab of that many MiB now; later requests are carved out of it first
 *                   (first fit, coalesced on release) and only fall back to hipMalloc when it cannot serve them —
 *                   a one-shot caller pays its device allocations here, not inside its first call
 *   "pool_guard"    1: every device block the ctx allocates from now on carries 256 canary bytes behind the bytes
 *                   its user asked for, verified (after a device synchronisation) when the block is released
 *   "pool_guard_check"  verifies the canaries of all live blocks now; CPH_ERR_INVALID + the first violation's
 *                   description if any canary was ever overwritten
 * Unknown names fail with CPH_ERR_INVALID. */
CPH_API int32_t cph_ctx_set_option(cph_ctx* ctx, const char* name, int64_t value);

/* Blocks until everything enqueued by this ctx has finished. */
CPH_API int32_t cph_ctx_synchronize(cph_ctx* ctx);

/* Pinned (page-locked) host staging memory: cgo must not hand Go-heap pointers
 * that C retains, and pinned buffers make H2D/D2H copies asynchronous.
 * Page-locking costs ~90 us per block — more than a Join of a batch of 8192 rows (60-80 us) — so blocks of at most 4 MB
 * handed back through cph_pinned_free are kept by the ctx (up to 32) and handed out again; a host side may allocate and
 * free its staging per batch (round 5; before, only a caller that kept its blocks — the Go shim's stagePool — avoided it).
 * A block must not be freed while a call that reads or writes it is still in flight (cph_stream_join_submit ... next). */
CPH_API int32_t cph_pinned_alloc(cph_ctx* ctx, size_t bytes, void** out);
CPH_API int32_t cph_pinned_free(cph_ctx* ctx, void* p);

/* ---- index build: IndexOn / UniqueIndexOn (csvplus.go:529-537, 707-756) ----- */

/*
 * Builds the sorted index over `nkeycols` key columns (all with the same
 * nrows), leftmost column most significant.
 *
 *   unique != 0  mirrors createUniqueIndex: if two rows have equal keys the
 *                call returns CPH_ERR_DUPLICATE and *first_dup_pos is the
 *                smallest sorted position i>=1 with rows[i-1]==rows[i] on the
 *                key columns (the pair csvplus.go:749-753 reports; the shim
 *                formats rows[perm[i]] into the error text of :751).  The index
 *                is still returned so the shim can read perm[i]; it must destroy
 *                it to mirror the reference's nil return.
 *   unique == 0  *first_dup_pos is still filled (UINT64_MAX when all keys are
 *                distinct); duplicates are not an error.
 *
 * The index stays resident on the GPU (sorted key codes + permutation).
 */
CPH_API int32_t cph_index_build(cph_ctx* ctx, const cph_strcol* keycols, int32_t nkeycols, int32_t unique,
                                cph_index** out, uint64_t* first_dup_pos);
/*
 * Several IndexOn calls as one batch (the two build sides of orders.Join(customers).Join(products),
 * README.md:56): the same results as nspecs calls of cph_index_build, but the batch pays the build's two
 * host round trips (key statistics, first duplicate) ONCE instead of once per index, and the kernels of the
 * different indexes queue back to back.  out[i] / first_dup_pos[i] / status[i] are per index (status and
 * first_dup_pos may be NULL); the return value is the first non-OK status (CPH_ERR_DUPLICATE for a `unique`
 * spec with equal keys — that index is still returned, as by cph_index_build).
 */
typedef struct cph_index_spec {
    const cph_strcol* keycols;
    int32_t           nkeycols;
    int32_t           unique;
} cph_index_spec;
CPH_API int32_t cph_index_build_many(cph_ctx* ctx, const cph_index_spec* specs, int32_t nspecs, cph_index** out,
                                     uint64_t* first_dup_pos, int32_t* status);
CPH_API void    cph_index_destroy(cph_index* index);

/* Number of rows / key columns of the index. */
CPH_API uint64_t cph_index_nrows(const cph_index* index);
CPH_API int32_t  cph_index_nkeycols(const cph_index* index);

/* perm[i] = original row id of the row at sorted position i.
 * mem = CPH_MEM_HOST: copied to library-owned pinned memory on first use;
 * mem = CPH_MEM_DEVICE: the resident device array.  Valid until destroy. */
CPH_API int32_t cph_index_perm(cph_index* index, int32_t mem, const uint32_t** perm, uint64_t* n);

/* ---- probe: Join / Except (csvplus.go:545-608) ------------------------------ */

/*
 * Probes `nprobecols` columns (1 <= nprobecols <= index key columns; fewer =
 * prefix join on the leading index columns, matched positionally,
 * csvplus.go:546-550, :910) against the index.
 *
 *   row_sel     optional (may be NULL): nsel row numbers into the probe columns,
 *               as uint32 (sel_bits = 32) or uint64 (sel_bits = 64) values from
 *               which sel_base is subtracted; probe row i is then row
 *               row_sel[i] - sel_base of the columns and nprobe = nsel.  Same
 *               memory space as the columns.  This is how a chained Join
 *               (README.md:56) stays on the device: the second probe passes the
 *               first join's probe_idx array (sel_bits = 64, sel_base = the first
 *               call's probe_base) and so probes exactly the rows the first join
 *               emitted, in emission order.
 *   probe_base  added to the local probe position in probe_idx (global row
 *               number of this chunk / shard's first row).
 *   want_pairs  0: only lo/cnt/nmatches are produced (Except, counting);
 *               1: probe_idx/build_row are expanded too.
 *   out_mem     where the result arrays should live.
 */
CPH_API int32_t cph_join_probe(cph_ctx* ctx, const cph_index* index, const cph_strcol* probecols,
                               int32_t nprobecols, const void* row_sel, int32_t sel_bits, uint64_t sel_base,
                               uint64_t nsel, uint64_t probe_base, int32_t want_pairs, int32_t out_mem,
                               cph_matches** out);
CPH_API void    cph_matches_release(cph_matches* m);

/* ---- chained Join on the device (README.md:56; csvplus.go:545-569 nested) ---- */

/* Joins per device call.  Chains of up to 4 Joins over duplicate-free single-column indexes run as ONE fused pass over the stream
 * rows; longer ones (and chains with duplicate keys / several key columns) run the general chain — probe, select, compose, one
 * step at a time — on the device, still inside one call (round 5: was 4, a fifth Join started a second call). */
#define CPH_MAX_CHAIN 8

/* One Join of a chain: stream.Join(index, cols...).  ncols <= the index's key columns.
 *   source == 0   `cols` are columns of the STREAM table (all such steps see the same nrows): the value the Join reads when
 *                 the stream row carries the column (mergeRows lets the stream's value win, csvplus.go:571-583).
 *   source == k   (1 <= k <= this step's number) `cols` are columns of the BUILD TABLE of step k-1 — the table steps[k-1].index
 *                 was built from, in that table's ORIGINAL row order (cols[j].nrows == cph_index_nrows(steps[k-1].index)): the
 *                 key of this Join is read from the row that step k-1 matched.  This is the reference's flagship chain,
 *                 people.Join(orders, "id").Join(products) (csvplus_test.go:280-285): prod_id is a column of the ORDERS index
 *                 row, which mergeRows copied into the joined row the second Join sees.
 *   source == -k  the same with `cols` laid out in step k-1's SORTED order (row i of cols = the row at sorted position i:
 *                 how the reference holds index.impl.rows after createIndex, csvplus.go:736; what cph_index_permute produces);
 *                 needs CPH_CHAIN_POSITIONS.
 * Step 0 always reads the stream. */
typedef struct {
    const cph_index*  index;
    const cph_strcol* cols;
    int32_t           ncols;
    int32_t           source;
} cph_chain_step;

/*
 * Result of stream.Join(i0, c0).Join(i1, c1)...: the joined rows as row-id tuples
 * in the reference's emission order (stream order; for one stream row the
 * matches of step 0 ascending by index position, and for each of them the
 * matches of step 1, ...).  stream_row[m] = probe_base + the stream row
 * (stream_row == NULL means the identity: every stream row joined exactly once, so
 * row m of the result is stream row probe_base + m and no array is materialised),
 * build_row[k][m] = ORIGINAL row id of the matching row of step k's index.
 * The host materialises row m as mergeRows(...mergeRows(index_k row, ...), stream row)
 * (csvplus.go:571-583).  Arrays live in `mem`, valid until cph_chain_release.
 */
typedef struct {
    uint64_t        nrows;
    const uint64_t* stream_row;
    const uint32_t* build_row[CPH_MAX_CHAIN];
    int32_t         nsteps;
    int32_t         mem;
    int32_t         positions;      /* 1: build_row[k][m] is the SORTED POSITION of the row in index k (see below) */
    int32_t         reserved_;
} cph_chain;

/*
 * A key of a later step is either a column of the stream table (source == 0) or a column of an earlier step's build table
 * (source != 0, see cph_chain_step) — between them the two cover every value mergeRows can hand to a later Join.  When every
 * index has distinct keys over a single column the whole chain runs as ONE pass over the stream rows, whatever the sources
 * (a build-side key is gathered from the matched row inside the kernel); otherwise the steps run one after the other ON THE
 * DEVICE (probe, expand, compose), still one call.
 */
CPH_API int32_t cph_join_chain(cph_ctx* ctx, const cph_chain_step* steps, int32_t nsteps, uint64_t probe_base,
                               int32_t out_mem, cph_chain** out);

/*
 * The same with flags.  CPH_CHAIN_POSITIONS: build_row[k][m] is not the original row id but the SORTED POSITION of the
 * matching row in index k — the value the reference itself works with: after createIndex the rows of an Index ARE in
 * sorted order (csvplus.go:736) and Join reads index.impl.rows[first() + i] (csvplus.go:553-567), so a host that keeps
 * its index rows sorted (as the reference does) reaches the joined row with one array access; the original row id is
 * cph_index_perm(index)[position].  For the device this removes the one random access per probe row that cannot be
 * cached: a duplicate-free index over a dense code space maps code -> position through presence bits and a running count
 * per 32 codes (8 bytes per 32 codes: 2.5 MB for a 1e7-code space, resident in every XCD's L2) instead of a 4-byte
 * row id per code (40 MB: one 64-byte Infinity-Fabric sector per probe row).
 */
#define CPH_CHAIN_POSITIONS 1u
CPH_API int32_t cph_join_chain_ex(cph_ctx* ctx, const cph_chain_step* steps, int32_t nsteps, uint64_t probe_base,
                                  int32_t out_mem, uint32_t flags, cph_chain** out);
CPH_API void    cph_chain_release(cph_chain* chain);

/* ---- multi-GPU: the exchange step of the row-range sharded Join ----- */

/*
 * One process (rank) per GPU joins a contiguous range of the stream rows against replicated build
 * sides; concatenating the per-rank row-id lists in rank order gives the reference's emission order
 * (stream order, csvplus.go:553-567).  A cph_dist wraps the communicator that moves those lists:
 * RCCL over xGMI (librccl.so is resolved on first use — the library does not link against it; a copy the host
 * process already loaded, e.g. torch's, is the one it binds to).
 *   rank 0:  cph_dist_unique_id(ctx, id)  -> ship the CPH_DIST_ID_BYTES bytes to every rank by any side
 *            channel the host program has (a Go host: its own RPC; torch: broadcast_object_list)
 *   all:     cph_dist_create(ctx, id, rank, nranks, &d)            (collective: ncclCommInitRank)
 * Every call below is collective: all ranks call it, in the same order, each on its own ctx.
 * Work is enqueued on the ctx's stream; the only host wait is for 24 bytes of counts per rank.
 */
#define CPH_DIST_ID_BYTES 128
#define CPH_MAX_GATHER    8
typedef struct cph_dist cph_dist;

CPH_API int32_t cph_dist_unique_id(cph_ctx* ctx, uint8_t* id /* CPH_DIST_ID_BYTES */);
CPH_API int32_t cph_dist_create(cph_ctx* ctx, const uint8_t* id, int32_t rank, int32_t nranks, cph_dist** out);
/* Test transport: the `nranks` ranks of `group` are THREADS of this process (one ctx each) sharing a GPU;
 * the collectives rendezvous in host memory and copy device to device.  Same code path above the transport. */
CPH_API int32_t cph_dist_create_loopback(cph_ctx* ctx, const char* group, int32_t rank, int32_t nranks, cph_dist** out);
CPH_API void    cph_dist_destroy(cph_dist* d);
CPH_API int32_t cph_dist_rank(const cph_dist* d);
CPH_API int32_t cph_dist_size(const cph_dist* d);
/* What moves the bytes, for logs and benchmark records: "rccl nranks=8 lib=<path> (the copy the host process had
 * loaded)" — the library binds to a librccl the process has ALREADY mapped (torch ships one) before it opens its
 * own, so one process never runs two RCCL copies — or "loopback nranks=...".  Owned by `d`, valid until the next call.
 * Environment: CPH_RCCL_LIBRARY=<path> makes the library bind to exactly that file (a particular RCCL build). */
CPH_API const char* cph_dist_transport(cph_dist* d);

/* Result of an allgatherv: data[a] (device memory of this rank's ctx, library-owned) holds `total`
 * elements of array a — rank 0's, then rank 1's, ...; counts / displs (host) say where each rank's begin.
 * Valid in stream order on the ctx's stream (cph_ctx_synchronize before reading from the host). */
typedef struct {
    uint64_t        total;
    int32_t         narrays, nranks;
    const uint64_t* counts;
    const uint64_t* displs;
    void*           data[CPH_MAX_GATHER];
    int32_t         mem;            /* CPH_MEM_DEVICE, or CPH_MEM_HOST: the arrays lie in the communicator's shared host
                                       buffer (cph_dist_join_chain with CPH_DIST_HOST_GATHER) */
    int32_t         reserved_;
} cph_gathered;

/* allgatherv of `narrays` device arrays that all hold `count` elements on this rank (elem_bytes[a] each):
 * ONE count exchange and ONE grouped send/recv batch for all arrays. */
CPH_API int32_t cph_dist_allgatherv(cph_dist* d, const void* const* send, const int32_t* elem_bytes, int32_t narrays,
                                    uint64_t count, cph_gathered** out);
CPH_API void    cph_gathered_release(cph_gathered* g);

/* The same for a chain result in device memory (cph_join_chain(..., probe_base, CPH_MEM_DEVICE)): gathers
 * build_row[0..nsteps) — data[0..nsteps) when *identity == 1: every rank's rows are its whole contiguous range,
 * so gathered row m is stream row *stream_base + m — or stream_row first (data[0], uint64) and the build rows
 * behind it (data[1..nsteps]) when some stream row of some rank did not join. */
CPH_API int32_t cph_dist_chain_allgather(cph_dist* d, const cph_chain* chain, uint64_t probe_base, cph_gathered** out,
                                         int32_t* identity, uint64_t* stream_base);

/*
 * The sharded chained Join in ONE call, its exchange pipelined behind the compute (round 4; csvplus.go:553-567 — rows are
 * independent, so a shard may be cut anywhere).  `steps` describe THIS rank's shard of the stream (its rows are stream rows
 * [probe_base, probe_base + nrows)); every rank passes the same chain.  The shard is cut into `nchunks` sub-chunks (0: the
 * library picks — one chunk per 2^24 rows of the largest shard, 1..8, and ONE for a single-rank communicator that keeps the result
 * on the device; the same value on every rank) and chunk k's rows travel while chunk k+1 is being joined:
 *   - default: to every peer over xGMI (RCCL send/recv batches on a second stream), straight into their final place in
 *     the gathered arrays — every rank ends up with the whole list in device memory, as with cph_dist_chain_allgather;
 *   - CPH_DIST_HOST_GATHER: each rank copies its chunks device -> host into ITS range of one host buffer that all ranks
 *     of the node share (POSIX shared memory, registered with HIP; created on first use and kept): no xGMI traffic at all,
 *     N PCIe links in parallel, and the joined list ends where a host program consumes it.  out->mem == CPH_MEM_HOST; the
 *     arrays stay valid until THIS rank's next CPH_DIST_HOST_GATHER call on the communicator or cph_dist_destroy (results
 *     alternate between two halves of the buffer, so a faster rank's next call does not touch what this rank still reads).
 * The pipeline needs results of a known size: a chain of duplicate-free single-column indexes yields at most one tuple per
 * stream row, so chunks travel in the dense form (slot == stream row) and the match totals are exchanged once at the end —
 * the call's only host wait; when some row of some rank did not join, the slots are compacted afterwards (one local pass).
 * Any other chain is joined whole and exchanged like cph_dist_chain_allgather does (stats->chunks == 0).
 *   shard_rows   optional: the row counts of ALL ranks' shards (nranks entries) when the caller knows them — as it does for
 *                a range split — and the ranges follow each other in rank order; NULL: one more count exchange up front.
 *   flags        CPH_CHAIN_POSITIONS (see cph_join_chain_ex) | CPH_DIST_HOST_GATHER | CPH_DIST_PACKED
 *   identity / stream_base / out: as cph_dist_chain_allgather.
 */
#define CPH_DIST_HOST_GATHER 0x100u
/* (round 6) xGMI mode only: the chunks travel BIT-PACKED — ceil(log2(index rows)) bits per step and row instead of 32 (the benchmark's
 * chain: 24 + 17 = 41 bits instead of 64), packed by the sender behind every sub-chunk's join, unpacked by the receiver behind the
 * exchange; the gathered arrays are the same.  Ignored (the plain format travels) when a row needs more than 64 bits, with
 * CPH_DIST_HOST_GATHER and for a single rank.  stats->packed_bits says what travelled. */
#define CPH_DIST_PACKED 0x200u
typedef struct {
    int32_t  chunks;               /* sub-chunks per shard; 0: the one-shot path ran                                      */
    int32_t  pipelined;            /* 1: more than one chunk, exchange and compute on separate streams                    */
    double   compute_ms;           /* ctx stream: first chunk's join enqueued -> last chunk's join done                   */
    double   exchange_ms;          /* exchange stream: first chunk ready -> match totals of all ranks received            */
    double   exposed_exchange_ms;  /* last chunk's join done -> totals received: the part of the exchange nothing hides   */
    double   total_ms;             /* first chunk's join enqueued -> totals received                                      */
    uint64_t bytes_sent, bytes_received;   /* this rank, row arrays only (xGMI; host gather: bytes_sent = PCIe bytes)     */
    int32_t  packed_bits;          /* CPH_DIST_PACKED in effect: bits per row on the wire; 0: plain 32 bits per step        */
    int32_t  reserved_;
} cph_dist_join_stats;
CPH_API int32_t cph_dist_join_chain(cph_dist* d, const cph_chain_step* steps, int32_t nsteps, uint64_t probe_base,
                                    const uint64_t* shard_rows, int32_t nchunks, uint32_t flags, cph_gathered** out,
                                    int32_t* identity, uint64_t* stream_base, cph_dist_join_stats* stats /* may be NULL */);

/* Build side, option B: rank `root` built `root_index` (others pass NULL); every other rank
 * receives an equal index (*out; NULL on the root) — descriptor, sorted codes and perm travel by ncclBroadcast
 * (12 bytes per row for one-word 64-bit codes) instead of every rank sorting the same table. */
CPH_API int32_t cph_dist_index_broadcast(cph_dist* d, const cph_index* root_index, int32_t root, cph_index** out);

/* ---- streaming Join of a host-resident stream (BASELINE config 5) -------------- */

/*
 * The probe side of a Join is a stream (csvplus.go:545-569 never materialises it).
 * When it lives in host memory it is fed chunk by chunk through a pipeline of
 * `nslots` slots, each with its own HIP stream, so that consecutive chunks overlap
 * upload, compute and download.
 *
 * cph_stream_join_create — chains the fused kernel accepts (every index has distinct
 * keys over ONE key column; CPH_ERR_INVALID otherwise): a submitted chunk's H2D copy,
 * kernels and D2H copy are enqueued without any host synchronisation.  Results are
 * DENSE per chunk (cph_stream_chunk.dense = 1): row r of the chunk joined iff bit
 * (r % 64) of match_bitmap[r / 64] is set, and then build_row[k][r] is the original
 * row id in index k.  Emission order is row order.  nmatches = number of set bits.
 *
 * cph_stream_join_create_general — ANY chain cph_join_chain takes (duplicate keys on
 * the build side, several key columns per step, prefix joins, keys of any length):
 * ncols[k] stream columns are step k's key, submit() takes the steps' columns one
 * after the other (ncols[0] + ncols[1] + ... columns).  The size of such a result is
 * only known after the probe, so every slot also owns a worker thread that runs the
 * general chain on the slot's stream; the pipeline overlaps across slots as before.
 * Results are PAIR LISTS per chunk (dense = 0), exactly cph_chain's layout:
 * nmatches joined rows in the reference's emission order, stream_row[m] (NULL: the
 * identity probe_base + m) and build_row[k][m]; match_bitmap is NULL.  A chain the
 * fused kernel accepts runs in the dense mode here as well.
 */
typedef struct cph_stream_join cph_stream_join;

typedef struct {
    uint64_t        probe_base;     /* as passed to submit                              */
    uint64_t        nrows;          /* rows of the chunk                                */
    uint64_t        nmatches;
    const uint64_t* match_bitmap;   /* ceil(nrows/1024)*16 words (>= nrows bits)        */
    const uint32_t* build_row[CPH_MAX_CHAIN];
    int32_t         nsteps;
    int32_t         dense;          /* 1: bitmap + one build row per chunk row; 0: pair lists of nmatches rows */
    const uint64_t* stream_row;     /* dense = 0: probe_base + chunk row of every joined row (NULL: identity)  */
    int32_t         positions;      /* 1: build_row[k] holds sorted positions in index k (cph_stream_join_set_positions) */
    int32_t         reserved_;
} cph_stream_chunk;

CPH_API int32_t cph_stream_join_create(cph_ctx* ctx, const cph_index* const* indexes, int32_t nsteps, int32_t nslots,
                                       cph_stream_join** out);
CPH_API int32_t cph_stream_join_create_general(cph_ctx* ctx, const cph_index* const* indexes, const int32_t* ncols,
                                               int32_t nsteps, int32_t nslots, cph_stream_join** out);
/* on != 0: every later chunk reports SORTED POSITIONS in build_row[k] instead of original row ids (CPH_CHAIN_POSITIONS,
 * see cph_join_chain_ex).  Call before the first submit. */
CPH_API int32_t cph_stream_join_set_positions(cph_stream_join* sj, int32_t on);
CPH_API void    cph_stream_join_destroy(cph_stream_join* sj);
/* step_cols[k] = the chunk's key column for step k: HOST memory (pinned — cph_pinned_alloc —
 * for real overlap), borrowed until the chunk has been returned by cph_stream_join_next.
 * Fails with CPH_ERR_INVALID when all slots are in flight. */
CPH_API int32_t cph_stream_join_submit(cph_stream_join* sj, const cph_strcol* step_cols, uint64_t probe_base);

/*
 * Key codes formed on the host (round 4): a stream in host memory then crosses PCIe as 4 bytes per row and step instead of
 * its key strings (17 bytes per row for the benchmark's two keys).  A stream row's key takes part in a Join only through
 * its code under the index's key codec, so for an index whose keys code in ONE word below 2^31 (cph_index_info:
 * code_words == 1, code_bits <= 31, dict_entries == 0, split == 0 — decimal ids, short tags) the host can form the code
 * with the table the device walks:
 *   cph_host_encoder_create   an encoder for `index` with a pool of `nthreads` worker threads (0: one per hardware
 *                             thread); CPH_ERR_INVALID when the index's codes do not qualify (ship the strings then)
 *   cph_host_encoder_run      cols = ALL key columns of the index for the chunk's rows (host memory) -> out_codes[nrows];
 *                             a key that cannot occur in the index gets CPH_CODE_ABSENT and joins nothing.  Blocks.
 *   cph_stream_join_submit_codes   like cph_stream_join_submit with step_codes[k] = the chunk's codes for step k (host
 *                             memory, pinned for real overlap; borrowed until the chunk was returned).  Fused-mode stream
 *                             joins only (cph_stream_join_create), every index with a direct lookup structure (dense code
 *                             space: cph_index_info.direct_table); results as for cph_stream_join_submit.
 * An encoder may be used from one thread at a time; it does not touch the GPU.
 */
#define CPH_CODE_ABSENT 0xFFFFFFFFu
typedef struct cph_host_encoder cph_host_encoder;
CPH_API int32_t cph_host_encoder_create(const cph_index* index, int32_t nthreads, cph_host_encoder** out);
CPH_API int32_t cph_host_encoder_threads(const cph_host_encoder* enc);
CPH_API int32_t cph_host_encoder_run(cph_host_encoder* enc, const cph_strcol* cols, int32_t ncols, uint32_t* out_codes);
CPH_API void    cph_host_encoder_destroy(cph_host_encoder* enc);
CPH_API int32_t cph_stream_join_submit_codes(cph_stream_join* sj, const uint32_t* const* step_codes, uint64_t nrows, uint64_t probe_base);
CPH_API int32_t cph_stream_join_pending(const cph_stream_join* sj);
/* Waits for the OLDEST chunk in flight.  The arrays are pinned memory owned by the
 * pipeline.  Slots are used round robin — chunk number k (counting submissions from 0)
 * lives in slot k % nslots — so the arrays of chunk k stay valid until chunk k + nslots
 * is SUBMITTED: a caller that keeps at most nslots - 1 chunks in flight can read a
 * returned chunk while the following ones are being processed. */
CPH_API int32_t cph_stream_join_next(cph_stream_join* sj, cph_stream_chunk* out);

/* ---- materialisation: the step after the path ------------------ */

/* A library-owned string column (64-bit offsets) living in col.mem. */
typedef struct {
    cph_strcol col;
    uint64_t   nbytes;      /* total value bytes */
} cph_colbuf;

/* A library-owned byte buffer. */
typedef struct {
    const uint8_t* data;
    uint64_t       size;
    int32_t        mem;
    int32_t        reserved_;
} cph_bytes;

/*
 * out[i] = col[row_ids[i] - id_base] for i < nrows (row_ids == NULL: a plain copy of
 * the column).  This is mergeRows (csvplus.go:571-583) column by column: a joined
 * table consists of the stream's columns (gathered through stream_row / probe_idx,
 * or used as they are when that is the identity) and of every index's columns
 * gathered through build_row; on a column-name collision the caller keeps the
 * stream's column (the stream value wins, :578-580).  row_ids are uint32
 * (id_bits 32) or uint64 (64) and live in the same memory space as the column.
 */
CPH_API int32_t cph_gather_rows(cph_ctx* ctx, const cph_strcol* col, const void* row_ids, int32_t id_bits,
                                uint64_t id_base, uint64_t nrows, int32_t out_mem, cph_colbuf** out);
CPH_API void    cph_colbuf_release(cph_colbuf* c);

/*
 * A column of the table an index was built over, in INDEX ORDER: out[p] = col[perm[p]] for the index's sorted
 * positions p (cph_gather_rows through cph_index_perm).  The reference's Index holds its rows sorted (createIndex,
 * csvplus.go:736) and Join reads index.impl.rows[first() + i]; a device pipeline that keeps the payload columns of a
 * build table in this order once (IndexOn time) consumes the sorted positions a Join reports (cph_join_chain_ex
 * CPH_CHAIN_POSITIONS, cph_stream_join_set_positions) directly as row subscripts — in cph_gather_rows, in
 * cph_csv_write_rows' cph_rowsel — and never needs the original row ids.  col must have the rows of the indexed table
 * (col->nrows > every perm value) and lives in host or device memory like the columns of cph_gather_rows.
 */
CPH_API int32_t cph_index_permute(cph_ctx* ctx, cph_index* index, const cph_strcol* col, int32_t out_mem, cph_colbuf** out);

/*
 * ToCsv (csvplus.go:379-406): the canonical serialisation — a header line (when
 * `header` != NULL: ncols names) and one record per row with the columns in the
 * given order, formatted as Go's encoding/csv Writer does with default settings
 * (',' separator, '\n' record end; a field is quoted iff it is `\.`, contains
 * ',', '"', '\r' or '\n', or starts with a Unicode space; '"' is doubled inside
 * quotes).  All columns must have the same number of rows.
 */
CPH_API int32_t cph_csv_write(cph_ctx* ctx, const cph_strcol* cols, int32_t ncols, const cph_strval* header,
                              int32_t out_mem, cph_bytes** out);

/*
 * Join(...).ToCsv(...) without materialising the joined table: output row i takes field c from row
 * sel[c].ids[i] - sel[c].base of cols[c] (sel == NULL or sel[c].ids == NULL: row i itself, and then
 * cols[c].nrows must equal nrows unless nrows is 0).  This is mergeRows (csvplus.go:571-583) folded into the writer:
 * the caller lists, per output column, the table it comes from (for a name present on both sides the
 * stream's column, :578-580) and the row-id array of that table from cph_join_chain / cph_join_probe.
 * Row ids live in the same memory space as their column and must be < cols[c].nrows.
 */
typedef struct {
    const void* ids;      /* uint32 or uint64 row ids, nrows entries; NULL = identity */
    int32_t     bits;     /* 32 or 64 */
    int32_t     reserved_;
    uint64_t    base;     /* subtracted from every id (e.g. the probe_base of a chunk) */
} cph_rowsel;

CPH_API int32_t cph_csv_write_rows(cph_ctx* ctx, const cph_strcol* cols, const cph_rowsel* sel, int32_t ncols, uint64_t nrows,
                                   const cph_strval* header, int32_t out_mem, cph_bytes** out);
CPH_API void    cph_bytes_release(cph_bytes* b);

/*
 * ToJSON (csvplus.go:446-480) over the same rows as cph_csv_write_rows: cols and sel mean exactly what they mean there
 * (per-column uint32 / uint64 row ids with a base; sel == NULL or sel[c].ids == NULL: the identity, and then cols[c].nrows
 * must equal nrows; host or device columns), names[c] is the key of column c.  The text is what the reference writes:
 * '[', then every row as json.Encoder.Encode(row) writes it with SetIndent("", "") and SetEscapeHTML(false) — a compact
 * object followed by '\n' — with ',' in front of every row but the first, then ']'.  n rows:
 *     [{"k1":"v1","k2":"v2"}\n,{"k1":"v1","k2":"v2"}\n]        (no spaces; nrows == 0 gives exactly "[]")
 * A Row is a map[string]string, so the keys of every object are sorted by byte order (the function sorts the columns by
 * name itself; the order the caller lists them in does not matter).  Keys and values are escaped as Go >= 1.22
 * encoding/json does with escapeHTML false:
 *   - 0x20..0x7F other than '"' and the backslash are copied (DEL, '<', '>', '&' included); those two get a backslash in front;
 *   - 0x08 0x0C 0x0A 0x0D 0x09 -> \b \f \n \r \t (Go before 1.22 wrote \u0008 and \u000c); other bytes < 0x20 -> \u00XX,
 *     lowercase hex;
 *   - bytes >= 0x80 are decoded as utf8.DecodeRuneInString does: a valid sequence is copied unchanged (a literal U+FFFD
 *     too), U+2028 / U+2029 become \u2028 / \u2029, an invalid or truncated sequence (overlong forms, surrogates, leads
 *     C0 C1 F5..FF, stray continuation bytes) becomes \ufffd and decoding resumes ONE byte later.
 * CPH_ERR_INVALID: names == NULL, ncols outside 1..16, two equal names (a map holds each key once: the caller resolves
 * mergeRows collisions, :578-580), row-id bits other than 32 / 64, an identity column whose row count is not nrows.
 * The result (out_mem HOST or DEVICE) is released with cph_bytes_release; its size is exact.
 */
CPH_API int32_t cph_json_write_rows(cph_ctx* ctx, const cph_strcol* cols, const cph_rowsel* sel, const cph_strval* names,
                                    int32_t ncols, uint64_t nrows, int32_t out_mem, cph_bytes** out);

/* ---- Filter / TakeWhile / DropWhile / Top / Drop with the named predicates (csvplus.go:276-374, :1243-1293) ---- */
/*
 * The reference's declarative predicates — Like (:1277-1293), All (:1243-1253), Any (:1258-1268), Not (:1271-1275) — as a
 * small POSTFIX PROGRAM over the columns of a call, so that any nesting of the four is one flat host array.  Every op
 * works on a stack of booleans, evaluated per row:
 *   CPH_PRED_LIKE  push (value of column `arg` of this row == value); arg = -1: the row has no such column, push false
 *                  (:1286 `!found`).  Equality is bytewise on the whole value: same length, same bytes, any byte value
 *                  (NUL included); the empty literal equals the empty value.
 *   CPH_PRED_NOT   pop a, push !a
 *   CPH_PRED_ALL   pop `arg` operands, push their AND; arg == 0 pushes true
 *   CPH_PRED_ANY   pop `arg` operands, push their OR;  arg == 0 pushes false
 * Like(Row{"a": x, "b": y}) is  LIKE a x, LIKE b y, ALL 2.  A program must leave exactly one value.  Limits (checked):
 * at most CPH_PRED_MAX_OPS ops, at most CPH_PRED_MAX_LIKE LIKE ops, a stack of at most CPH_PRED_MAX_STACK values; the
 * literal of a LIKE may have any length.
 *
 * Numeric compare terms — the reference's `year, _ := row.ValueAsInt("born"); return year > 1970` (csvplus_test.go:272-281)
 * as data:
 *   CPH_PRED_INT_LT .. CPH_PRED_INT_GT (16..21, in the order LT LE EQ NE GE GT)   push (int64 of column `arg`)   REL literal
 *   CPH_PRED_FLT_LT .. CPH_PRED_FLT_GT (24..29, same order)                       push (float64 of column `arg`) REL literal
 * `value` points at exactly 8 host bytes: the int64_t or the double literal.  The column's value is converted as
 * cph_col_to_number converts it; a row that does NOT convert (syntax, range, unsupported) pushes FALSE under every
 * relation, NE included — what the reference's closure does with the error — and arg = -1 (no such column) pushes false.
 * Float relations are IEEE: with a NaN on either side only NE holds.  A numeric term counts against CPH_PRED_MAX_LIKE
 * like a LIKE term.
 *
 * String terms that look INSIDE a value — `row["ts"] >= "2016-09"`, `strings.HasPrefix(row["ts"], "2016-09-14")`,
 * `strings.Contains(row["surname"], "Smith")` as data:
 *   CPH_PRED_STR_LT .. CPH_PRED_STR_GT (32..37, in the order LT LE EQ NE GE GT)   push strings.Compare(value of column `arg`, literal) REL 0
 *   CPH_PRED_HAS_PREFIX (40)   push strings.HasPrefix(value, literal)
 *   CPH_PRED_HAS_SUFFIX (41)   push strings.HasSuffix(value, literal)
 *   CPH_PRED_CONTAINS   (42)   push strings.Contains(value, literal)
 * `arg` is the column and `value` the literal's bytes exactly as for CPH_PRED_LIKE: host memory, any length below 4 GiB, any
 * byte values, a NULL pointer allowed with len == 0.  These are BYTE operations, as in Go.  Compare is bytewise and unsigned
 * ("\x7f" < "\x80", "10" < "9"), and of two values that agree on their common prefix the shorter is the smaller ("a" <
 * "a\0").  An empty literal holds for every present value under PREFIX / SUFFIX / CONTAINS, the empty value included; a
 * literal longer than the value fails all three.  arg = -1 (no such column) pushes FALSE under every one of the nine ops, NE
 * included — the rule of LIKE and of the numeric terms.  CONTAINS is a per-row search whose worst case is quadratic in the
 * value's length (a value that repeats the literal's first byte and mismatches late).
 *
 * Time terms — `t, err := time.Parse(time.RFC3339, row["ts"]); return err == nil && !t.Before(start)` as data:
 *   CPH_PRED_TIME_LT .. CPH_PRED_TIME_GT (48..53, in the order LT LE EQ NE GE GT)   push (t.Unix() of column `arg`) REL (u.Unix() of the literal)
 * `value` is the literal as RFC 3339 TEXT (host memory); the host converts it with the routine the device runs.  A literal
 * that does not convert with CPH_NUM_OK (cph_col_to_number, CPH_NUM_TIME_UNIX) fails the call with CPH_ERR_INVALID, and so does
 * a literal with a fraction: the term compares WHOLE SECONDS, a fraction would mislead.  The column is converted first through
 * the path of cph_col_to_number (once per column and call); a row that does not convert pushes FALSE under every relation, NE
 * included, and arg = -1 pushes false.  Two stamps of the same instant in different zones are equal here, which their bytes
 * (CPH_PRED_STR_*) are not.
 *
 * Expression terms — `price(r) * float64(qty(r)) >= 100`, `died(r) > born(r)` as data: two cph_num_eval expressions compared:
 *   CPH_PRED_EXPR_LT .. CPH_PRED_EXPR_GT (56..61, in the order LT LE EQ NE GE GT)   push (lhs of this row) REL (rhs of this row)
 * `value.data` points at ONE cph_pred_expr in host memory (declared behind cph_expr_nums below) and value.len ==
 * sizeof(cph_pred_expr).  Its program is a cph_num_eval program that leaves exactly TWO values of ONE type, lhs below rhs; COL_*
 * leaves index this call's cols, and entry p of a number array belongs to POSITION p of the selection (first_row included), so
 * an array has at least first_row + nrows entries.  Typing is checked on the host with cph_num_eval's rules; int64 and float64
 * do not mix across the relation either (no implicit conversions).  int64 compares signed; float64 compares IEEE: with a NaN
 * on either side only NE holds, and -0 == +0.  A row in which ANY op fails — a leaf that does not convert, a zero divisor, a
 * TO_INT out of range — pushes FALSE under every relation, NE included (what the reference's closure does with err: the rule
 * of INT_* / FLT_*).  `arg` is 0; arg = -1 means "a column of the expression is not in the rows": the term is false and `value`
 * is ignored.  One kernel (k_expr_cmp) reads the leaves once and writes one BIT per row; a program that consists of a single
 * expression term runs nothing else in the WHERE mode.  Deferred float leaves take cph_num_eval's two routes, with the same bits.
 *
 * Column-against-column terms — `r["ship_city"] != r["bill_city"]` as data:
 *   CPH_PRED_COLS_LT .. CPH_PRED_COLS_GT (72..77, same order)   push strings.Compare(value of column `arg`, value of column b) REL 0
 * `value.data` points at 4 host bytes holding the int32_t column b and value.len == 4.  These are exactly CPH_PRED_STR_*'s rules
 * with the second value in the literal's place: bytewise, unsigned, the shorter of two values that agree on the common prefix
 * the smaller.  Either column -1 pushes FALSE under all six relations.  The two columns may have different layouts (fixed width,
 * 32- / 64-bit offsets) and different row ids: that is how a joined row compares a stream column with a build column.
 *
 * Every LIKE, numeric, string, time, expression and column-against-column term counts against CPH_PRED_MAX_LIKE (32 terms in
 * all).  The valid ops are 1..4, 16..21, 24..29, 32..37, 40..42, 48..53, 56..61 and 72..77; every other op (0, 5..15, 22, 23, 30,
 * 31, 38, 39, 43..47, 54, 55, 62..71, 78..) is invalid.
 *
 * Out of scope for a condition: boolean-valued ops and math functions inside an expression, string operands inside an
 * expression, prefix / suffix / contains against another column; case mapping (it needs Go's Unicode tables: a project of
 * its own); a condition on a trimmed or split value directly (map it first: a CPH_MAP_SPAN piece of cph_map_format gives an
 * ordinary column); regular expressions; time layouts other than RFC 3339, named zones, and comparing below the second.
 */
enum { CPH_PRED_LIKE = 1, CPH_PRED_NOT = 2, CPH_PRED_ALL = 3, CPH_PRED_ANY = 4 };
enum { CPH_PRED_INT_LT = 16, CPH_PRED_INT_LE = 17, CPH_PRED_INT_EQ = 18, CPH_PRED_INT_NE = 19, CPH_PRED_INT_GE = 20, CPH_PRED_INT_GT = 21 };
enum { CPH_PRED_FLT_LT = 24, CPH_PRED_FLT_LE = 25, CPH_PRED_FLT_EQ = 26, CPH_PRED_FLT_NE = 27, CPH_PRED_FLT_GE = 28, CPH_PRED_FLT_GT = 29 };
enum { CPH_PRED_STR_LT = 32, CPH_PRED_STR_LE = 33, CPH_PRED_STR_EQ = 34, CPH_PRED_STR_NE = 35, CPH_PRED_STR_GE = 36, CPH_PRED_STR_GT = 37 };
enum { CPH_PRED_HAS_PREFIX = 40, CPH_PRED_HAS_SUFFIX = 41, CPH_PRED_CONTAINS = 42 };
enum { CPH_PRED_TIME_LT = 48, CPH_PRED_TIME_LE = 49, CPH_PRED_TIME_EQ = 50, CPH_PRED_TIME_NE = 51, CPH_PRED_TIME_GE = 52, CPH_PRED_TIME_GT = 53 };
enum { CPH_PRED_EXPR_LT = 56, CPH_PRED_EXPR_LE = 57, CPH_PRED_EXPR_EQ = 58, CPH_PRED_EXPR_NE = 59, CPH_PRED_EXPR_GE = 60, CPH_PRED_EXPR_GT = 61 };
enum { CPH_PRED_COLS_LT = 72, CPH_PRED_COLS_LE = 73, CPH_PRED_COLS_EQ = 74, CPH_PRED_COLS_NE = 75, CPH_PRED_COLS_GE = 76, CPH_PRED_COLS_GT = 77 };
#define CPH_PRED_MAX_OPS   64
#define CPH_PRED_MAX_LIKE  32
#define CPH_PRED_MAX_STACK 32
typedef struct {
    int32_t    op;      /* CPH_PRED_* */
    int32_t    arg;     /* LIKE / INT_* / FLT_* / STR_* / HAS_* / CONTAINS / TIME_* / COLS_*: column (index into cols) or -1; EXPR_*: 0 or -1;
                           ALL / ANY: operand count; NOT: ignored */
    cph_strval value;   /* LIKE / STR_* / HAS_* / CONTAINS: the literal's bytes; INT_* / FLT_*: 8 bytes, an int64_t / a double; TIME_*: RFC 3339 text;
                           EXPR_*: one cph_pred_expr; COLS_*: 4 bytes, the int32_t second column; host memory */
} cph_pred_op;

enum { CPH_FILTER_WHERE = 0, CPH_FILTER_TAKE_WHILE = 1, CPH_FILTER_DROP_WHILE = 2 };
typedef struct {
    int32_t  mode;       /* CPH_FILTER_WHERE       Filter(pred):    the rows where pred holds (:276-286)
                            CPH_FILTER_TAKE_WHILE  TakeWhile(pred): the rows before the first row where it fails (:346-358)
                            CPH_FILTER_DROP_WHILE  DropWhile(pred): that row and all rows after it (:362-374)            */
    int32_t  out_bits;   /* 32 or 64: width of the row numbers written                                                */
    uint64_t first_row;  /* the call looks at rows [first_row, first_row + nrows) of the selection:
                            src.Drop(first_row).Top(nrows) IN FRONT of the filter (:313-342)                          */
    uint64_t skip;       /* .Drop(skip) BEHIND the filter                                                             */
    uint64_t limit;      /* .Top(limit) behind that; UINT64_MAX = no limit                                            */
} cph_filter_opts;

/* An ascending list of row numbers; library-owned until cph_rowlist_release. */
typedef struct {
    uint64_t    nrows;
    uint64_t    first;   /* ids == NULL: the list is the range first, first + 1, ... (the two WHILE modes always answer
                            this way: nothing is materialised)                                                        */
    const void* ids;     /* `bits`-wide row numbers in `mem`, ascending = the reference's emission order              */
    int32_t     bits, mem;
} cph_rowlist;

/*
 * cols / sel / nrows mean exactly what they mean for cph_csv_write_rows and cph_json_write_rows (host or device columns,
 * fixed-width or 32 / 64-bit offsets, per-column uint32 / uint64 row ids with a base, living where the column lives), so
 * a predicate can be evaluated over JOINED rows without materialising them.  The only difference: the call looks at the
 * selection's rows [first_row, first_row + nrows), so an identity column needs at least first_row + nrows rows (rather
 * than exactly nrows) and a row-id array at least that many entries.  ncols may be 0 (and cols NULL) for a program
 * without LIKE terms over real columns.  The row numbers written are POSITIONS IN THAT SELECTION (they include first_row),
 * i.e. directly usable as cph_rowsel.ids / row_ids / row_sel of every consumer whose columns are identity columns.
 * The predicate's strings are read once (one evaluation kernel per call); WHERE keeps a bitmap of one bit per row between
 * its two kernels.  The result is complete when the call returns (the other calls' rule).
 *
 * CPH_ERR_INVALID (with a message in cph_last_error): NULL ctx / prog / opts / out, cols NULL with ncols > 0, nops outside
 * 1..CPH_PRED_MAX_OPS, an unknown op, a LIKE / numeric / string-term column outside -1..ncols-1, a LIKE or string-term value
 * with a length but no pointer, a string-term literal of 4 GiB or more,
 * a numeric literal that is not exactly 8 bytes behind a non-NULL pointer, a time literal that is no whole-second RFC 3339 stamp,
 * an expression term whose value is not exactly one cph_pred_expr, whose prog is NULL, whose nops is outside
 * 2..CPH_EXPR_MAX_OPS, whose nnums is outside 0..CPH_EXPR_MAX_NUMS (or nums NULL with nnums > 0, a number array without values
 * or with an unknown memory space), whose program breaks a rule of cph_num_eval or does not leave exactly two values of one
 * type, or whose arg is neither 0 nor -1; a column-against-column term whose value is not exactly 4 bytes or whose either
 * column is outside -1..ncols-1,
 * a negative or too large ALL / ANY count (stack underflow), a NOT on an empty stack, a program that does not leave
 * exactly one value, the limits above, out_bits or row-id bits other than 32 / 64, an unknown mode or out_mem, a short
 * identity column.  CPH_ERR_TOO_MANY_ROWS when out_bits == 32 and first_row + nrows > 2^32 - 1, and when nrows alone is
 * (the count of kept rows is a 32-bit number).  nrows == 0 is legal and yields an empty list.
 */
CPH_API int32_t cph_filter_rows(cph_ctx* ctx, const cph_strcol* cols, const cph_rowsel* sel, int32_t ncols, uint64_t nrows,
                                const cph_pred_op* prog, int32_t nops, const cph_filter_opts* opts, int32_t out_mem,
                                cph_rowlist** out);
CPH_API void    cph_rowlist_release(cph_rowlist* list);

/*
 * The companion for consumers whose columns are NOT identity columns: out[i] = sel->ids[list[i]] - sel->base — a plain
 * gather, as wide as sel->ids, base 0 — which is how the per-column row ids of a Join are narrowed to the rows a Filter
 * kept.  sel == NULL or sel->ids == NULL (the identity) returns a copy of the list (a range stays a range).  sel->ids
 * live in sel_mem and must have more entries than the list's largest row number; a list in the other memory space is
 * copied across first.  The result lives in out_mem.
 */
CPH_API int32_t cph_rowsel_take(cph_ctx* ctx, const cph_rowsel* sel, int32_t sel_mem, const cph_rowlist* list, int32_t out_mem,
                                cph_rowlist** out);

/* ---- Row.ValueAsInt / Row.ValueAsFloat64 for a whole column (csvplus.go:165-205) ---- */
/*
 * One string column, read through an optional row selection, as int64 or float64 with the semantics of Go's strconv
 * (restated here from its published behaviour; the reference tree pins only the two error strings, csvplus_test.go:911-958).
 *
 * CPH_NUM_INT64 = strconv.Atoi on a 64-bit int, decided left to right: "", "+", "-" are syntax errors; one optional
 * '+' / '-', then one or more '0'..'9' (any number of leading zeros; "-0" is 0) is the value; any other byte met BEFORE
 * the unsigned accumulator overflows 2^64 is a syntax error (value 0); the overflow itself is a range error AT THAT BYTE
 * (later bytes are not looked at: "99999999999999999999x" is a range error, "9223372036854775808x" a syntax error);
 * a fully parsed magnitude >= 2^63 without '-', or > 2^63 with it, is a range error.  Range errors carry INT64_MAX, or
 * INT64_MIN after '-'.
 *
 * CPH_NUM_FLOAT64 = strconv.ParseFloat(s, 64): [+-]?inf, [+-]?infinity and nan (no sign), ASCII case-insensitive; else
 * [+-]? ( D+ [ . D* ] | . D+ ) ( [eE] [+-]? D+ )?; everything else is a syntax error (value 0).  The result is the
 * correctly rounded double (a zero mantissa gives +-0; underflow to 0 or a denormal is no error); a magnitude beyond the
 * largest double is a range error with value +-Inf.  A value that contains '_' or starts 0x / 0X after the sign gets
 * CPH_NUM_ERR_UNSUPPORTED and value 0: Go may accept it (digit separators, hexadecimal floats), this library does not
 * decide — a stated limit, never a silent wrong answer.  The device converts every value whose mantissa (the first 19
 * significant digits, none dropped but zeros) is below 2^53 and whose decimal exponent lies in -22..37 (Clinger's exact
 * cases: one IEEE operation); the other valid rows are finished on the library's host side, and `host_rows` counts them.
 * With cph_ctx_set_option "float_device" = 1 the device also converts those other rows (Eisel-Lemire: any mantissa of up to 19
 * digits with any exponent, overflow to a range error with +-Inf and underflow to +-0 or a denormal included) and hands on only
 * the ones that conversion leaves undecided — values with non-zero digits behind the 19th whose two neighbours w and w + 1 round
 * differently, under 1 % of such values; `host_rows` then counts exactly those.  The results are the same bits either way.
 *
 * CPH_NUM_TIME_UNIX / CPH_NUM_TIME_UNIXNANO = `t, err := time.Parse(time.RFC3339, s)` followed by t.Unix() (whole seconds
 * since 1970-01-01T00:00:00Z, the FLOOR: "1969-12-31T23:59:59.5Z" is -1) / t.UnixNano(); both write int64_t[nrows], and
 * host_rows is always 0.  The reference pins nothing about timestamps, so the accepted set is the strict RFC 3339 profile
 * that time.Parse(time.RFC3339, s) and Time.UnmarshalText accept with the same meaning.  With D a byte '0'..'9' the value
 * must be, in full:   DDDD-DD-DDTDD:DD:DD  [ '.' D{1,9} ]  ( 'Z' | ('+'|'-') DD:DD )
 * A row's status is decided in this order:
 *   1. CPH_NUM_ERR_UNSUPPORTED  the value matches only after one or more of these relaxations: the hour written with one
 *      digit ("...T8:48:22Z"), ',' in place of the fraction's '.', more than 9 fraction digits.  Go's lenient Parse accepts or
 *      truncates these and Go versions differ on them; this library does not decide (the stance of '_' and 0x above).
 *   2. CPH_NUM_ERR_SYNTAX       every other value that does not match: "", a lower-case t or z, a blank for the T, a missing
 *      zone, "+0100", '.' without digits, trailing bytes.
 *   3. CPH_NUM_ERR_RANGE        month outside 1..12, day outside 1..days(month, year) (proleptic Gregorian; year 0000 is valid
 *      and a leap year), hour > 23, minute > 59, second > 59 ("23:59:60" is a range error, as in Go).
 *   4. CPH_NUM_ERR_UNSUPPORTED  zone hour > 23 or zone minute > 59.
 *   5. CPH_NUM_ERR_UNSUPPORTED  CPH_NUM_TIME_UNIXNANO only: the result does not fit an int64 (before 1677-09-21T00:12:43.145224192Z
 *      or after 2262-04-11T23:47:16.854775807Z); Go documents UnixNano as undefined there.
 * The value at every error row is 0.  The instant is civil(date, time) - offset; "-00:00" is offset 0; years 0000..9999 all
 * fit CPH_NUM_TIME_UNIX.  Other layouts, named zones and DST rules are out of scope.
 *
 * A conversion error is DATA: the call returns CPH_OK and the struct says what failed.  col / sel / nrows mean what they
 * mean for cph_csv_write_rows with one column (host or device, fixed-width or 32 / 64-bit offsets, optional row ids with
 * a base: a Join's output converts without being materialised).  CPH_ERR_INVALID (with a message): NULL ctx / col / out,
 * an unknown kind or out_mem, row-id bits other than 32 / 64, an identity column whose row count is not nrows.
 * nrows == 0 is legal (values and status are NULL).
 */
enum { CPH_NUM_INT64 = 1, CPH_NUM_FLOAT64 = 2, CPH_NUM_TIME_UNIX = 4, CPH_NUM_TIME_UNIXNANO = 5 };   /* 0, 3: invalid */
enum { CPH_NUM_OK = 0, CPH_NUM_ERR_SYNTAX = 1, CPH_NUM_ERR_RANGE = 2, CPH_NUM_ERR_UNSUPPORTED = 3 };
typedef struct {
    uint64_t       nrows;
    const void*    values;          /* int64_t[nrows] (INT64, TIME_*) or double[nrows], in `mem`; what Go returns beside the error at error rows */
    const uint8_t* status;          /* CPH_NUM_* per row, in `mem` */
    int32_t        kind, mem;
    uint64_t       nerrors;
    uint64_t       first_error_row; /* position in the selection; UINT64_MAX when nerrors == 0 */
    int32_t        first_error_kind, reserved_;
    uint64_t       host_rows;       /* float only: rows finished on the host */
} cph_numcol;
CPH_API int32_t cph_col_to_number(cph_ctx* ctx, const cph_strcol* col, const cph_rowsel* sel, uint64_t nrows, int32_t kind,
                                  int32_t out_mem, cph_numcol** out);
CPH_API void    cph_numcol_release(cph_numcol* col);

/* ---- Numeric expressions per row: price * float64(qty) (csvplus_test.go:516-571, :1391-1421) ---- */
/*
 * The reference's numeric flows convert two columns of a (joined) row and do arithmetic on them in a Go closure:
 * `price * float64(qty)`.  A closure cannot run on a GPU; a small typed POSTFIX PROGRAM can.  Every op works on a stack of
 * int64 / float64 values, evaluated per output row i:
 *   CPH_EXPR_COL_INT   push strconv.Atoi(value of column `arg` in this row)          -> int64   (cph_col_to_number's rules)
 *   CPH_EXPR_COL_FLT   push strconv.ParseFloat(value of column `arg`, 64)            -> float64 (likewise)
 *   CPH_EXPR_NUM_INT   push ((const int64_t*)nums[arg].ptr)[i]                       -> int64
 *   CPH_EXPR_NUM_FLT   push ((const double*)nums[arg].ptr)[i]                        -> float64
 *   CPH_EXPR_LIT_INT / CPH_EXPR_LIT_FLT   push lit.i / lit.f
 *   CPH_EXPR_TO_FLT    float64(x) of an int64: rounded to nearest, ties to even
 *   CPH_EXPR_TO_INT    int64(x) of a float64: truncation toward zero
 *   CPH_EXPR_NEG       -x;   CPH_EXPR_ADD SUB MUL DIV: pop b, pop a, push a OP b;   CPH_EXPR_MOD: the same, int64 only
 * Columns are read through their row ids as everywhere (cols / sel / ncols / nrows mean exactly what they mean for
 * cph_map_format: host or device columns, fixed-width or 32 / 64-bit offsets, one cph_rowsel per column, so a Join's output
 * evaluates without being materialised).  A number array has nrows entries in nums[k].mem (CPH_MEM_HOST / CPH_MEM_DEVICE; a
 * host array is staged) and entry i belongs to OUTPUT row i — it is not read through row ids, like the pieces of Map.
 *
 * Typing is Go's: there are no implicit conversions.  The host checks the program before anything is launched: ADD SUB MUL
 * DIV take two operands of the same type, MOD and TO_FLT take int64, TO_INT takes float64, NEG takes either, and exactly
 * one value must be left — its type is the result's `kind`.
 *
 * Arithmetic.  int64: ADD SUB MUL NEG wrap in two's complement; DIV truncates toward zero and MOD has the dividend's sign
 * (-7 / 2 == -3, -7 % 2 == -1, 7 / -2 == -3, 7 % -2 == 1); INT64_MIN / -1 == INT64_MIN and INT64_MIN % -1 == 0 (the Go
 * specification, not a trap).  A zero divisor — a run-time panic in Go — is DATA here: status CPH_NUM_ERR_DIV_ZERO, value 0.
 * float64: every op is ONE correctly rounded IEEE operation; a product feeding a sum is never contracted into a fused
 * multiply-add (Go on amd64 never fuses); division by zero gives +-Inf or NaN as IEEE says and is no error.
 * TO_INT of a NaN or of a value outside [-2^63, 2^63) is CPH_NUM_ERR_CONVERT with value 0: Go leaves that conversion
 * implementation-defined and this library does not guess (the stance of CPH_NUM_ERR_UNSUPPORTED).
 *
 * Errors are DATA, as for cph_col_to_number: the call returns CPH_OK and the result says what failed.  A COL_* leaf that does
 * not convert carries cph_col_to_number's status for that value.  Within one row the FIRST failing op in program order
 * decides the row's status (the reference's closure returns at its first error); later ops do not matter.  An error row
 * holds value 0.  nerrors counts rows; first_error_row is the lowest failing row, first_error_kind its status, and
 * *first_error_op (may be NULL) the index of the op that failed there, -1 without errors — what a host needs to name the
 * column in its message.
 *
 * The result is an ordinary cph_numcol (released with cph_numcol_release): kind = the program's result type, values and
 * status per row in out_mem; it plugs into CPH_MAP_INT64 / CPH_MAP_FLOAT64 pieces and cph_agg_spec.numbers unchanged.
 * One kernel reads the strings once and writes 9 bytes per row.  The float rows the device defers (cph_col_to_number) make
 * the call convert every string leaf by that entry point's route first — the host finishing included — and evaluate over
 * the converted arrays; both routes give the same bits, and host_rows counts the rows with a deferred float leaf.
 *
 * CPH_ERR_INVALID (with a message in cph_last_error, *out stays NULL): NULL ctx / prog / out, cols NULL with ncols > 0, nums
 * NULL with nnums > 0, ncols outside 0..16, nops outside 1..CPH_EXPR_MAX_OPS, nnums outside 0..CPH_EXPR_MAX_NUMS, an unknown
 * op, a COL_* arg outside 0..ncols-1, a NUM_* arg outside 0..nnums-1, a number array that is NULL while nrows > 0 or has an
 * unknown memory space, a type violation, an operand missing, a stack deeper than CPH_EXPR_MAX_STACK, a program that does
 * not leave exactly one value, an unknown out_mem, row-id bits other than 32 / 64, an identity column whose row count is
 * not nrows.  nrows == 0 is legal (values and status are NULL).
 *
 * Out of scope: boolean results (comparing two expressions is a term of cph_filter_rows: CPH_PRED_EXPR_*, over the
 * cph_pred_expr below), math functions and rounding helpers, string operands, more than one result per call.
 */
enum { CPH_NUM_ERR_DIV_ZERO = 4, CPH_NUM_ERR_CONVERT = 5 };   /* beside CPH_NUM_OK .. CPH_NUM_ERR_UNSUPPORTED = 0..3 */
enum { CPH_EXPR_COL_INT = 1, CPH_EXPR_COL_FLT = 2, CPH_EXPR_NUM_INT = 3, CPH_EXPR_NUM_FLT = 4, CPH_EXPR_LIT_INT = 5,
       CPH_EXPR_LIT_FLT = 6, CPH_EXPR_TO_FLT = 8, CPH_EXPR_TO_INT = 9, CPH_EXPR_NEG = 10, CPH_EXPR_ADD = 11, CPH_EXPR_SUB = 12,
       CPH_EXPR_MUL = 13, CPH_EXPR_DIV = 14, CPH_EXPR_MOD = 15 };
#define CPH_EXPR_MAX_OPS   32
#define CPH_EXPR_MAX_STACK 8
#define CPH_EXPR_MAX_NUMS  8
typedef struct {
    int32_t op;    /* CPH_EXPR_* */
    int32_t arg;   /* COL_*: index into cols; NUM_*: index into nums; otherwise ignored */
    union { int64_t i; double f; } lit;   /* LIT_INT / LIT_FLT */
} cph_expr_op;
typedef struct {
    const void* ptr;   /* int64_t[nrows] or double[nrows]; entry i belongs to OUTPUT row i */
    int32_t     mem;   /* CPH_MEM_HOST / CPH_MEM_DEVICE */
    int32_t     reserved_;
} cph_expr_nums;
/* The value of a CPH_PRED_EXPR_* term of cph_filter_rows / cph_map_switch (see there): two expressions in one program. */
typedef struct {
    const cph_expr_op*   prog;   /* a cph_num_eval program that leaves exactly TWO values of ONE type: lhs below rhs */
    int32_t              nops;   /* 2..CPH_EXPR_MAX_OPS for both sides together; stack <= CPH_EXPR_MAX_STACK */
    int32_t              nnums;
    const cph_expr_nums* nums;   /* entry p belongs to POSITION p of the selection: at least first_row + nrows entries */
} cph_pred_expr;

CPH_API int32_t cph_num_eval(cph_ctx* ctx, const cph_strcol* cols, const cph_rowsel* sel, int32_t ncols, uint64_t nrows,
                             const cph_expr_nums* nums, int32_t nnums, const cph_expr_op* prog, int32_t nops,
                             int32_t out_mem, cph_numcol** out, int32_t* first_error_op /* may be NULL */);

/* ---- Map with a row template: a computed string column (csvplus.go:290-296) ---- */
/*
 * The reference's Map takes a closure (`row["name"] = "Julia"`, `row["full"] = row["name"] + " " + row["surname"]`, the
 * README's Printf over a joined row); a closure cannot run on a GPU, a ROW TEMPLATE can: value i of the new column is the
 * concatenation, in order, of the template's pieces —
 *   CPH_MAP_LITERAL  the bytes of `value` (host memory, any length, any byte values);
 *   CPH_MAP_COLUMN   the value of column `arg` (an index into cols) in row i;
 *   CPH_MAP_INT64    ints[i] written as strconv.FormatInt(v, 10) does: '-' in front of a negative value, no '+', no leading
 *                    zeros, 0 gives "0", INT64_MIN its 20 characters.  `ints` has nrows entries in the memory space `arg`
 *                    (CPH_MEM_HOST / CPH_MEM_DEVICE); entry i belongs to OUTPUT row i (it is not read through row ids) —
 *                    e.g. the values of cph_col_to_number, or of cph_num_eval (an expression over the same rows).
 *   CPH_MAP_FLOAT64  floats[i] written as strconv.FormatFloat(v, 'f', prec, 64) does: an optional '-', the integer digits (at
 *                    least "0"), and with prec > 0 a '.' and exactly prec digits; rounded to nearest, ties to even, on the
 *                    EXACT binary value (2.675 at prec 2 gives "2.67", 2.5 at prec 0 "2", 0.125 at prec 2 "0.12").  The sign
 *                    stays when the result rounds to zero (-0.001 at prec 2: "-0.00"; -0.0: "-0", "-0.00").  NaN of any sign
 *                    or payload gives "NaN", the infinities "+Inf" and "-Inf".  `floats` has nrows entries in the memory
 *                    space `arg`, entry i belongs to OUTPUT row i, a host array is staged: all as for INT64.
 *                    Two limits: prec must be within 0..22, and a FINITE value with |v| >= 2^128 is not formatted — the call
 *                    fails with CPH_ERR_INVALID, the message names the piece and the LOWEST such output row, *out stays NULL
 *                    (infinities and NaN are not such values).  Inside both limits the digits are exact with 128-bit
 *                    integer arithmetic (the integer part is below 2^128, the scaled fraction below 2^53 * 10^22 < 2^127);
 *                    outside them the exact decimal digits need a big-number loop, which this does not have.
 *   CPH_MAP_SLICE    the bytes [from, to) of the value of column `arg` in row i — Go's `row["ts"][:10]`.  `value` points at
 *                    exactly 16 host bytes, a cph_map_slice {from, to}.  Python's slice rules: a negative index counts from
 *                    the value's end, both ends are then clamped into [0, len], from >= to gives the empty string, and
 *                    to == INT64_MAX means "to the end".  Bytes, not runes, as in Go.  One deviation: where Go panics on an
 *                    index out of range, this clamps.
 *   CPH_MAP_TIME     ints[i] = Unix seconds of OUTPUT row i (the rules of INT64: `arg` is the memory space, a host array is
 *                    staged, no row ids), written as time.Unix(v, 0).In(time.FixedZone("", 60 * prec)).Format(time.RFC3339)
 *                    does.  `prec` carries the zone as minutes east of UTC, -1439..1439: "YYYY-MM-DDTHH:MM:SSZ" (20 bytes) when
 *                    prec == 0, otherwise "YYYY-MM-DDTHH:MM:SS+HH:MM" / "-HH:MM" (25 bytes).  A value whose LOCAL year falls
 *                    outside 0000..9999 is not formatted: the call fails with CPH_ERR_INVALID, the message names the piece and
 *                    the LOWEST such output row, *out stays NULL — exactly as for the FLOAT64 limit.
 *   CPH_MAP_FLOAT64_SHORTEST  floats[i] written as strconv.FormatFloat(v, fmt, -1, 64) does, with the format byte fmt in `prec`:
 *                    one of 'e' 'E' 'f' 'g' 'G'.  `floats` and `arg` follow the rules of FLOAT64 (nrows entries, entry i belongs
 *                    to OUTPUT row i, a host array is staged).  The digits d1...dn (1..17 of them) are the SHORTEST that
 *                    strconv.ParseFloat maps back to the same double and, among strings of that length, the one closest
 *                    to the exact binary value (what fmt.Sprint, encoding/json, Python's repr and std::to_chars print).
 *                    With exp = the decimal exponent of d1:
 *                      'e' / 'E'  d1[.d2...dn]e±XX: no point when n = 1, at least two exponent digits, three when |exp| >= 100;
 *                                 at most 24 bytes ("-2.2250738585072014e-308").
 *                      'f'        no exponent.  |v| < 1: "0." , the zeros up to d1, the digits; otherwise the digits with the
 *                                 point inside them, or the digits and then zeros up to the units with no point.  At most 327
 *                                 bytes (the same value: '-', "0.", 307 zeros, 17 digits; 5e-324 is "0.", 323 zeros, "5");
 *                                 at most 310 for |v| >= 1.
 *                      'g' / 'G'  the 'e' / 'E' form when exp < -4 || exp >= 6, otherwise the 'f' form (Go decides with
 *                                 precision 6 for the shortest digits; 21 is %v's and JSON's threshold, not 'g''s); at most
 *                                 24 bytes.
 *                    Zero gives "0e+00", "0", "0" and -0 keeps its sign ("-0e+00", "-0", "-0"); NaN of any sign or payload gives
 *                    "NaN", the infinities "+Inf" and "-Inf".  Exact for every double (Schubfach, one 128-bit table entry per
 *                    value), and NO value is refused: 2^128 and 1e300 are formatted like any other.  The text reads back to
 *                    the same bits through cph_col_to_number.
 *   CPH_MAP_SPAN     the value of column `arg` in row i (read through its own row ids, like COLUMN and SLICE) NARROWED by a short
 *                    program of span operations: the result is a sub-span of the source value, no byte changes.  `value` points
 *                    at 1..CPH_SPAN_MAX_OPS cph_span_op in host memory; they are applied left to right, each to the span the
 *                    previous one left.  Each stands for a Go call, over bytes:
 *                      TRIM_SPACE    mode BOTH: strings.TrimSpace; LEFT / RIGHT: strings.TrimLeftFunc / TrimRightFunc(s,
 *                                    unicode.IsSpace).  Exact for every byte string, invalid UTF-8 included: a space is one of 25
 *                                    byte sequences — \t \n \v \f \r ' '; C2 85, C2 A0; E1 9A 80; E2 80 80 .. E2 80 8A; E2 80 A8,
 *                                    E2 80 A9, E2 80 AF; E2 81 9F; E3 80 80 — and from each end the longest run of them goes.  At
 *                                    the tail a sequence matches only together with its start byte (utf8.DecodeLastRune's
 *                                    decision): a lone 85 or 80 stops the trim, "E2 80 80 80" keeps its four bytes, "E2 C2 85"
 *                                    loses its last two.
 *                      TRIM_CUTSET   strings.Trim / TrimLeft / TrimRight(s, cutset) by mode.  The cutset is 0..32 bytes, all below
 *                                    0x80 (bytewise trimming is then Go's result for every byte string); the empty set changes
 *                                    nothing; a set byte of 0x80 or above is refused, never guessed.
 *                      TRIM_PREFIX / TRIM_SUFFIX   strings.TrimPrefix / TrimSuffix: once, and only if the literal (any bytes,
 *                                    0..255 of them) is there.
 *                      FIELD         parts = strings.Split(s, sep) for mode -1, strings.SplitN(s, sep, mode) for mode >= 1; the
 *                                    result is parts[a] for a >= 0 and parts[len(parts) + a] for a < 0.  One deviation, SLICE's
 *                                    kind: an index outside parts gives the empty span where Go panics.  strings.Cut falls out of
 *                                    it: `before` is field 0 of limit 2, `after` field 1 of limit 2 (empty when the separator is
 *                                    absent).  The separator is 1..255 bytes of any value, matched left to right without
 *                                    overlap ("aaa" on "aa": "", "a"); the empty value gives one empty field.
 *                      SLICE         bytes [a, b) of the current span under cph_map_slice's rules: TrimSpace(ts)[:10] is one piece.
 *                    The SPAN pieces of one call hold at most CPH_SPAN_MAX_TOTAL operations together; their literal bytes go
 *                    into the plan's literal block and count against its 4 GiB.  One lane runs one row's program: correct for
 *                    any value length, tuned for CSV-sized values.  Both passes compute the span; nothing is cached between them.
 * All bytes are copied verbatim (NUL and bytes >= 0x80 included); nothing is escaped.
 *
 * cols / sel / nrows mean exactly what they mean for cph_csv_write_rows (host or device columns, fixed-width or 32 / 64-bit
 * offsets, per-column uint32 / uint64 row ids with a base living where the column lives; an identity column must have
 * exactly nrows rows), so a template over JOINED rows reads every column through its own table's row ids and nothing is
 * materialised.  ncols may be 0 (and cols NULL) for a template without COLUMN pieces.
 *
 * The result is an ordinary library-owned cph_colbuf (64-bit offsets, in out_mem, released by cph_colbuf_release): an
 * identity column for every consumer — the writers, cph_filter_rows, cph_index_build.  nbytes is exact; nrows == 0 is
 * legal and yields an empty column.
 *
 * CPH_ERR_INVALID (with a message in cph_last_error): NULL ctx / pieces / out, npieces outside 1..CPH_MAP_MAX_PIECES, an
 * unknown kind (5..7, 9, 11, 13 and 15 included), a COLUMN, SLICE or SPAN index outside 0..ncols-1 (a column the rows lack is the host's business:
 * it substitutes a literal or reports the reference's missing-column error), a SLICE whose value is not exactly 16 bytes
 * behind a non-NULL pointer, a literal with a length but no pointer, an INT64 piece with ints ==
 * NULL while nrows > 0 or with an unknown memory space, a FLOAT64 piece with floats == NULL while nrows > 0, with an unknown
 * memory space or with prec outside 0..22, a FLOAT64 value beyond the range above (found while the call runs), a TIME piece with
 * ints == NULL while nrows > 0, with an unknown memory space or with prec outside -1439..1439, a TIME value whose local year is
 * outside 0000..9999 (found while the call runs), a FLOAT64_SHORTEST piece with floats == NULL while nrows > 0, with an unknown
 * memory space or with a prec that is none of 'e' 'E' 'f' 'g' 'G' (FLOAT64 with prec -1 stays refused: the shortest digits are
 * the other kind), a SPAN piece whose value is NULL or no whole number of cph_span_op, with 0 or more than CPH_SPAN_MAX_OPS
 * operations, or that brings the call beyond CPH_SPAN_MAX_TOTAL, a span operation with an unknown op or mode, with a literal
 * that has a length but no pointer or is over its limit (32 / 255 bytes), a cutset byte of 0x80 or above, an empty separator,
 * a FIELD limit of 0 or below -1, ncols outside 0..16 or cols NULL with ncols > 0, row-id bits other
 * than 32 / 64, an identity column whose row count is not nrows, an unknown out_mem.
 *
 * Out of scope: the remaining forms of FormatFloat — 'e' / 'g' with an explicit precision, 'b' / 'x', and 32-bit floats
 * (bitSize 32) —; case mapping (it changes bytes and needs Go's Unicode tables: a project of its own); a cutset with
 * a byte of 0x80 or above; splitting on the empty separator; regular expressions; a slice whose ends come from another column; time layouts other than RFC 3339, named
 * zones and DST rules.  A value that
 * depends on a condition is cph_map_switch's.
 */
enum { CPH_MAP_LITERAL = 1, CPH_MAP_COLUMN = 2, CPH_MAP_INT64 = 3, CPH_MAP_FLOAT64 = 4, CPH_MAP_SLICE = 8, CPH_MAP_TIME = 10,
       CPH_MAP_FLOAT64_SHORTEST = 12, CPH_MAP_SPAN = 14 };   /* 5..7, 9, 11, 13: invalid */
#define CPH_MAP_MAX_PIECES 16
typedef struct { int64_t from, to; } cph_map_slice;   /* what a SLICE piece's `value` points at: 16 bytes */
/* One operation of a SPAN piece (see CPH_MAP_SPAN above); a piece's `value` points at 1..CPH_SPAN_MAX_OPS of them. */
enum { CPH_SPAN_TRIM_SPACE = 1, CPH_SPAN_TRIM_CUTSET = 2, CPH_SPAN_TRIM_PREFIX = 3, CPH_SPAN_TRIM_SUFFIX = 4, CPH_SPAN_FIELD = 5,
       CPH_SPAN_SLICE = 6 };
enum { CPH_SPAN_LEFT = 1, CPH_SPAN_RIGHT = 2, CPH_SPAN_BOTH = 3 };   /* the mode of TRIM_SPACE / TRIM_CUTSET */
#define CPH_SPAN_MAX_OPS      4     /* operations in one SPAN piece */
#define CPH_SPAN_MAX_TOTAL    16    /* operations in the SPAN pieces of one call together (all alternatives of a switch) */
#define CPH_SPAN_MAX_CUTSET   32    /* bytes of a TRIM_CUTSET set, each below 0x80 */
#define CPH_SPAN_MAX_LITERAL  255   /* bytes of a TRIM_PREFIX / TRIM_SUFFIX literal (0..255) or of a FIELD separator (1..255) */
typedef struct {
    int32_t    op;    /* CPH_SPAN_* */
    int32_t    mode;  /* TRIM_SPACE / TRIM_CUTSET: CPH_SPAN_LEFT / RIGHT / BOTH; FIELD: SplitN's n, -1 (all) or >= 1; otherwise 0 */
    int64_t    a, b;  /* SLICE: from, to (cph_map_slice's rules); FIELD: a = the index k, b = 0; otherwise 0 */
    cph_strval lit;   /* TRIM_CUTSET: the set; TRIM_PREFIX / TRIM_SUFFIX: the literal; FIELD: the separator; host memory */
} cph_span_op;
typedef struct {
    int32_t        kind;    /* CPH_MAP_* */
    int32_t        arg;     /* COLUMN / SLICE / SPAN: index into cols; INT64 / FLOAT64 / FLOAT64_SHORTEST / TIME: memory space of `ints` / `floats` (CPH_MEM_*); LITERAL: ignored */
    cph_strval     value;   /* LITERAL: its bytes (host memory, any length, any byte values); SLICE: a cph_map_slice, len == 16;
                               SPAN: 1..CPH_SPAN_MAX_OPS cph_span_op, len == their number * sizeof(cph_span_op) */
    const int64_t* ints;    /* INT64 / TIME: nrows values, entry i belongs to OUTPUT row i (no row ids) */
    const double*  floats;  /* FLOAT64 / FLOAT64_SHORTEST: likewise */
    int32_t        prec;    /* FLOAT64: digits behind the point, 0..22; TIME: the zone, minutes east of UTC, -1439..1439; FLOAT64_SHORTEST: the format byte */
    int32_t        reserved_;
} cph_map_piece;

CPH_API int32_t cph_map_format(cph_ctx* ctx, const cph_strcol* cols, const cph_rowsel* sel, int32_t ncols, uint64_t nrows,
                               const cph_map_piece* pieces, int32_t npieces, int32_t out_mem, cph_colbuf** out);

/* ---- conditional Map: the template of the first case that holds (csvplus.go:290-296) ---- */
/*
 * The reference's Map closures branch: `if row["name"] == "Amelia" { row["name"] = "Julia" }` (csvplus_test.go:283-288).  As
 * data, that is a SWITCH: value i of the new column is the template of the FIRST case whose condition holds for row i, and
 * the template `otherwise` where none does — Go's if / else if / else, or switch { case ...: }.
 *
 * Columns.  cols / sel / nrows mean exactly what they mean for cph_map_format: an identity column has exactly nrows rows,
 * every column is read through its own row ids, so a Switch over JOINED rows materialises nothing.  The conditions and the
 * templates index the SAME cols array and share its limit of 16 columns.
 *
 * Conditions.  A case's `prog` is a cph_filter_rows program over cols, evaluated with first_row = 0: a LIKE or numeric term on
 * column -1 is false; a numeric term on a value that does not convert is false under every relation; float terms compare
 * the doubles cph_col_to_number produces, so an answer never depends on where a value was converted.  A float column several
 * cases compare is converted once per call.
 *
 * Selection.  Row i takes the alternative a = the lowest case index whose program holds, or ncases (`otherwise`) if none
 * does.  Its value is that alternative's pieces rendered exactly as cph_map_format renders them (LITERAL / COLUMN / INT64 /
 * FLOAT64 / FLOAT64_SHORTEST / SLICE / TIME / SPAN; verbatim bytes; FormatInt, FormatFloat and RFC 3339 rules).  which[i] = a when `which` is not NULL (nrows bytes of HOST
 * memory, written when the call succeeds).
 *
 * Number pieces.  INT64 / FLOAT64 / FLOAT64_SHORTEST / TIME arrays have nrows entries indexed by OUTPUT row.  Entries of rows that select ANOTHER
 * alternative are never interpreted and may hold anything; in particular the FLOAT64 refusal (a finite |v| >= 2^128) and the
 * TIME refusal (a local year outside 0000..9999) fail
 * the call only for a row that selects the alternative holding that piece.  The message then names the alternative, the
 * piece and the lowest such row, and *out stays NULL.  A FLOAT64_SHORTEST piece refuses no value, so it can never fail a row.
 *
 * Result.  An ordinary library-owned cph_colbuf: 64-bit offsets, exact nbytes, in out_mem.  nrows == 0 is legal, and so is a
 * call in which every row selects an empty value (nbytes == 0).
 *
 * CPH_ERR_INVALID, with a message in cph_last_error that names the case: NULL ctx / cases / otherwise / out; ncases outside
 * 1..CPH_MAP_MAX_CASES; a case with NULL prog or pieces; npieces / notherwise outside 1..CPH_MAP_MAX_PIECES; more than
 * CPH_MAP_SWITCH_MAX_PIECES pieces in all alternatives together; everything cph_filter_rows rejects in a program; everything
 * cph_map_format rejects in a piece or in the row sources.  CPH_ERR_TOO_MANY_ROWS for nrows > 2^32 - 1 (the predicate
 * evaluator's limit).
 *
 * Out of scope: nested switches; a conditional part inside a template (use one Switch over whole templates); case mapping; a non-ASCII cutset and an empty separator (SPAN pieces); regular expressions;
 * the other forms of FormatFloat; time layouts other than RFC 3339.
 */
#define CPH_MAP_MAX_CASES         8
#define CPH_MAP_SWITCH_MAX_PIECES 32      /* the pieces of all alternatives together */
typedef struct {
    const cph_pred_op*   prog;    int32_t nops;     /* the condition: a cph_filter_rows program over `cols` */
    const cph_map_piece* pieces;  int32_t npieces;  /* the value where this is the FIRST case that holds; 1..CPH_MAP_MAX_PIECES */
} cph_map_case;

CPH_API int32_t cph_map_switch(cph_ctx* ctx, const cph_strcol* cols, const cph_rowsel* sel, int32_t ncols, uint64_t nrows,
                               const cph_map_case* cases, int32_t ncases,                 /* 1..CPH_MAP_MAX_CASES */
                               const cph_map_piece* otherwise, int32_t notherwise,        /* 1..CPH_MAP_MAX_PIECES */
                               int32_t out_mem, cph_colbuf** out,
                               uint8_t* which /* NULL, or nrows bytes of HOST memory */);

/* ---- CSV ingest: bytes -> SoA string columns (csvplus.go:1080-1146) ----------- */
/*
 * Replaces the parse loop of Reader.Iterate (csv.NewReader + one map per line,
 * csvplus.go:1104-1131): the caller resolves the header to FIELD INDICES
 * (makeHeader, csvplus.go:1149-1206, stays on the host) and receives one
 * string column per requested index.  Semantics are Go's encoding/csv Reader
 * as csvplus configures it (csvplus.go:1088-1093): Comma, Comment,
 * TrimLeadingSpace, FieldsPerRecord; "\r\n" -> "\n"; empty and comment lines
 * skipped; `""` = literal quote.  cph_csv_parse rejects LazyQuotes = 1
 * (CPH_ERR_INVALID; cph_csv_parse_lazy takes it), and so it does a comment line
 * that contains a '"' (Go skips it uninterpreted; the parallel quote-parity scan
 * cannot — the state scan of cph_csv_parse_lazy can, and accepts such lines).
 *
 * cph_csv_parse_lazy = Reader.LazyQuotes() (csvplus.go:982-987): readRecord with
 * LazyQuotes = true.  A field whose first byte (after trimming, if on) is not '"'
 * is unquoted and runs to the next Comma or line end; quotes inside it are bytes
 * (`a""b` stays `a""b`).  In a quoted field `""` is one '"', '"' + Comma ends the
 * field, '"' + line end ("\n", "\r\n", the text's end, "\r" + the text's end) ends
 * field and record, '"' + anything else is a literal '"' and the field stays
 * quoted; a line end inside it is content (comment character and blank lines are
 * not looked at there), and the text's end inside it ends it silently.  There is
 * no ErrBareQuote and no ErrQuote: CPH_CSV_ERR_FIELD_COUNT is the only error_kind.
 * Everything else is as in cph_csv_parse.  One limit, detected: with
 * trim_leading_space, a field whose trimmed-off prefix holds a NON-ASCII Unicode
 * space (U+0085, U+00A0, U+1680, U+2000..) and whose next byte is '"' — Go reads
 * it as quoted, the device's separator scan trims ASCII spaces only — fails the
 * call with CPH_ERR_INVALID (the message names the case).  A record with fewer fields than a
 * requested index yields "" for that column — callers that want the
 * reference's "missing column" error (csvplus.go:1121-1124) set
 * fields_per_record > 0, as csvplus itself does with NumFields.
 */
enum {
    CPH_CSV_ERR_BARE_QUOTE  = 1,  /* csv.ErrBareQuote: '"' inside an unquoted field          */
    CPH_CSV_ERR_QUOTE       = 2,  /* csv.ErrQuote: stray or unterminated '"' in a quoted field */
    CPH_CSV_ERR_FIELD_COUNT = 3   /* csv.ErrFieldCount                                        */
};

typedef struct {
    uint8_t  comma;               /* Reader.delimiter (csvplus.go:1088); ASCII, not '"' '\r' '\n' */
    uint8_t  comment;             /* Reader.comment   (csvplus.go:1089); 0 = none                 */
    uint8_t  trim_leading_space;  /* csvplus.go:1092                                              */
    uint8_t  lazy_quotes;         /* csvplus.go:1091; 0 here; cph_csv_parse_lazy takes 1          */
    int32_t  fields_per_record;   /* csv.Reader.FieldsPerRecord: >0 exact, 0 = as the first record, <0 = any */
    uint64_t skip_records;        /* leading records to drop from the output (the header line; they are
                                     still parsed, validated and counted in error_record)          */
} cph_csv_options;

typedef struct {
    uint64_t   nrecords;          /* records returned: those before the first error, minus skip_records */
    uint64_t   error_record;      /* if error_kind != 0: 0-based record index (skipped records included) */
    int32_t    error_kind;        /* 0 or CPH_CSV_ERR_*: the first error in record order; the reference
                                     delivers the rows before it and then fails the same way           */
    int32_t    ncols;
    cph_strcol cols[CPH_MAX_KEY_COLS];   /* cols[i] = field col_index[i] of every record, in out_mem; offsets are
                                            32-bit when the text is smaller than 4 GiB, else 64-bit */
} cph_csv_table;

/* `data`/`size` = the whole CSV text in `mem` (CPH_MEM_HOST or CPH_MEM_DEVICE).
 * col_index[ncols] = 0-based field indices wanted, 1 <= ncols <= CPH_MAX_KEY_COLS. */
CPH_API int32_t cph_csv_parse(cph_ctx* ctx, const uint8_t* data, uint64_t size, int32_t mem, const cph_csv_options* opt,
                              const int32_t* col_index, int32_t ncols, int32_t out_mem, cph_csv_table** out);
/* The same call under LazyQuotes rules (above): opt->lazy_quotes must be 1, CPH_ERR_INVALID otherwise. */
CPH_API int32_t cph_csv_parse_lazy(cph_ctx* ctx, const uint8_t* data, uint64_t size, int32_t mem, const cph_csv_options* opt,
                                   const int32_t* col_index, int32_t ncols, int32_t out_mem, cph_csv_table** out);
CPH_API void    cph_csv_table_release(cph_csv_table* t);

/* ---- Find / SubIndex bounds (csvplus.go:870-891) ----------------------------- */

/* [*lower, *upper) = sorted positions whose leading key columns equal
 * `values` (nvalues <= key columns; 0 values = the whole index). */
CPH_API int32_t cph_index_find(cph_ctx* ctx, const cph_index* index, const cph_strval* values, int32_t nvalues,
                               uint64_t* lower, uint64_t* upper);

/* Many Find / SubIndex calls at once (csvplus.go:625-641 in a loop, e.g. BenchmarkSearchSmallSingleIndex,
 * csvplus_test.go:1104-1116): key k is values[k * nvalues .. (k + 1) * nvalues); lower[k] / upper[k] as cph_index_find.
 * One upload, ONE kernel launch and one download for the whole batch instead of a launch and two waits per key. */
CPH_API int32_t cph_index_find_many(cph_ctx* ctx, const cph_index* index, const cph_strval* values, int32_t nvalues,
                                    uint64_t nkeys, uint64_t* lower, uint64_t* upper);

/* ---- ResolveDuplicates support + persistence (csvplus.go:643-705, :810-867) ---- */

/*
 * Every maximal run of >= 2 equal keys, ascending: group g = sorted positions
 * [lower[g], upper[g]).  This is what dedup (csvplus.go:810-867) discovers one
 * group at a time — the adjacent-equal scans :815-819 / :851-855 give
 * lower[g]+1, the sort.Search :828-830 gives upper[g].  The resolve callback
 * and the compaction rule (:823-860, including which rows survive) stay with
 * the caller; cph_index_select then builds the compacted index.
 * Arrays are host memory owned by the library until cph_groups_release.
 */
typedef struct {
    uint64_t        ngroups;
    const uint64_t* lower;
    const uint64_t* upper;
} cph_groups;

CPH_API int32_t cph_index_dup_groups(cph_ctx* ctx, const cph_index* index, cph_groups** out);
CPH_API void    cph_groups_release(cph_groups* g);

/* New index = the rows at the given sorted positions of `index` (host array,
 * strictly ascending, < nrows; CPH_ERR_INVALID otherwise): index.rows[:dest]
 * after dedup's in-place compaction (csvplus.go:845-863).  Row ids (perm) keep
 * referring to the original build table. */
CPH_API int32_t cph_index_select(cph_ctx* ctx, const cph_index* index, const uint64_t* positions, uint64_t n,
                                 cph_index** out);

/*
 * Index.ResolveDuplicates with a NAMED rule instead of a callback: the choice per group, the compaction of dedup
 * (csvplus.go:810-867) and the new index, all on the device — nothing crosses to the host per group or per row.
 *
 * The choice for a group [lo, hi) (a maximal run of >= 2 equal keys, as cph_index_dup_groups reports them):
 *   CPH_RESOLVE_FIRST  lo           CPH_RESOLVE_LAST  hi-1          CPH_RESOLVE_DROP  no row (the reference's empty row)
 *   CPH_RESOLVE_MIN / CPH_RESOLVE_MAX   the position whose ORDER VALUE is smallest / largest; ties go to the lowest position
 *     (the index order is stable, so "first" and "lowest position" mean: first in the input).
 * The order value of sorted position p is row perm[p] of `order_col`, a column of the BUILD TABLE in its original row order
 * (host or device, any cph_strcol layout, nrows >= the table's rows).  It is required for MIN / MAX and ignored — may be
 * NULL — for the other rules.  order_kind says how it is compared:
 *   CPH_NUM_INT64 / CPH_NUM_FLOAT64   converted exactly as cph_col_to_number converts it.  Floats: -0 equals +0 (a pair of them
 *                                     is a tie); a NaN loses to every number under MIN and under MAX alike, and a group of
 *                                     nothing but NaNs keeps lo.
 *   CPH_ORDER_BYTES                   the index's own comparison (csvplus.go:794-806, strings.Compare): unsigned bytewise, a
 *                                     proper prefix is smaller.
 * Survivors: every row outside a group, and every group's chosen row — with the reference's TAIL RULE: when ngroups > 0,
 * keep_last_row == 0 and the final sorted row n-1 is not inside a group, that row is dropped ([A,A,B] -> [A]; dedup copies
 * rows[lower-1] only while lower < len(rows), :851-859).  ngroups == 0 changes nothing.
 *
 * A group row whose order value does not convert is DATA, as in cph_col_to_number: the call returns CPH_OK with nerrors > 0,
 * nrows = 0, positions = NULL and *out_index = NULL; first_error_position is the lowest such sorted position,
 * first_error_row = perm[that], first_error_kind its CPH_NUM_ERR_*.  Rows OUTSIDE groups are never looked at for errors: the
 * reference's callback never sees them.
 *
 * *out_index (when out_index != NULL) = the compacted index, what cph_index_select builds over `positions`.
 * CPH_ERR_INVALID (with a message): NULL ctx / index / opts / out, an unknown rule, order kind or out_mem, MIN / MAX
 * without a column or with one shorter than the build table.  Indexes of 0 and 1 rows are legal.
 */
enum { CPH_RESOLVE_FIRST = 1, CPH_RESOLVE_LAST = 2, CPH_RESOLVE_DROP = 3, CPH_RESOLVE_MIN = 4, CPH_RESOLVE_MAX = 5 };
enum { CPH_ORDER_BYTES = 3 };            /* beside CPH_NUM_INT64 = 1, CPH_NUM_FLOAT64 = 2 */
typedef struct { int32_t rule, order_kind, keep_last_row, reserved_; } cph_resolve_opts;
typedef struct {
    uint64_t        nrows;               /* surviving rows */
    const uint64_t* positions;           /* their sorted positions in the INPUT index, ascending, in `mem` */
    int32_t         mem, reserved_;
    uint64_t        ngroups, group_rows; /* runs of >= 2 equal keys, and the rows inside them */
    uint64_t        nerrors;             /* rows INSIDE groups whose order value did not convert */
    uint64_t        first_error_position, first_error_row;   /* lowest such sorted position, perm[that]; UINT64_MAX */
    int32_t         first_error_kind, reserved2_;            /* CPH_NUM_ERR_* */
    uint64_t        host_rows;           /* float order: values finished on the host */
} cph_resolved;
CPH_API int32_t cph_index_resolve(cph_ctx* ctx, const cph_index* index, const cph_resolve_opts* opts, const cph_strcol* order_col,
                                  int32_t out_mem, cph_index** out_index /* may be NULL */, cph_resolved** out);
CPH_API void    cph_resolved_release(cph_resolved* r);

/*
 * Totals: one Count and up to CPH_AGG_MAX_SPECS Sum / Min / Max values per KEY of an index, on the device — the reduction the
 * reference's TestSimpleTotals (csvplus_test.go:516-571) writes as a Go closure over the rows.  A closure cannot run on a GPU;
 * the aggregate is data, as the rules of cph_index_resolve are.
 *
 * A GROUP is a maximal run of equal keys in the index; a run of ONE row is a group too (cph_index_dup_groups and
 * cph_index_resolve report only runs of >= 2).  Group g is in key order; inside a run the rows are in input order.
 *   first_position[g]  the sorted position of the run's first row, ascending: usable as `positions` of cph_index_select, which
 *                      then builds the unique index over the distinct keys;
 *   first_row[g]       perm[first_position[g]], the first INPUT row with that key: 32-bit row ids for cph_rowsel, so the key
 *                      columns of the result are a gather (cph_gather_rows, the writers), not a copy;
 *   count[g]           rows of the run;
 *   values[s][g]       spec s over the run: int64_t[ngroups] for CPH_NUM_INT64, double[ngroups] for CPH_NUM_FLOAT64.
 * All arrays lie in `mem` (= out_mem) and are owned by the library until cph_aggregated_release.
 *
 * The value of sorted position p for a spec is either row perm[p] of `col`, a column of the BUILD TABLE in its original row
 * order (host or device, any cph_strcol layout, nrows >= the table's rows) converted exactly as cph_col_to_number converts it,
 * or numbers[perm[p]] of an int64_t[] / double[] array with one entry per row of the build table (in numbers_mem).  Exactly
 * one of col / numbers is set.
 *   CPH_AGG_SUM  int64: two's-complement wrap-around, what Go's `+=` on an int does; never an error.
 *                float64: IEEE double addition; NaN and inf - inf propagate.  The association order is unspecified but FIXED:
 *                the same index and values give bit-identical sums on every call and for every out_mem (no floating-point
 *                atomics, nothing that depends on scheduling; the partials of a run that spans tiles are folded in ascending
 *                tile order).
 *   CPH_AGG_MIN / CPH_AGG_MAX  int64: exact.  float64: math.Min / math.Max as documented — Min(-0, +0) = -0, Max(-0, +0) = +0,
 *                and a NaN anywhere in the run gives NaN (also beside an infinity); the NaN returned has the bits of Go's
 *                math.NaN().  Both are associative and commutative: the order does not matter.
 *
 * A `col` value that does not convert is DATA, as in cph_col_to_number / cph_index_resolve: the call returns CPH_OK with
 * nerrors > 0 (the number of such values over all specs), ngroups = 0 and every array NULL; first_error_position is the lowest
 * such sorted position (EVERY row lies in a group here, so every row is looked at), first_error_row = perm[that],
 * first_error_kind its CPH_NUM_ERR_*, first_error_spec the lowest spec that fails there.  `numbers` cannot have errors.
 * Floats outside Clinger's exact cases are finished on the library's host side as everywhere else (host_rows).
 *
 * nspecs == 0 is legal (specs may be NULL): groups, first rows and counts only — "the distinct keys and their frequencies".
 * Indexes of 0 and 1 rows are legal, and so is every index cph_index_resolve accepts (32-bit, one-word and multi-word codes,
 * several key columns, indexes out of cph_index_select / cph_index_resolve / cph_index_load).
 * CPH_ERR_INVALID (with a message): NULL ctx / index / out, nspecs outside 0..CPH_AGG_MAX_SPECS, specs NULL with nspecs > 0,
 * an unknown op, kind, numbers_mem or out_mem, both or neither of col / numbers, a col shorter than the build table.
 */
enum { CPH_AGG_SUM = 1, CPH_AGG_MIN = 2, CPH_AGG_MAX = 3 };
#define CPH_AGG_MAX_SPECS 8
typedef struct {
    int32_t           op, kind;              /* CPH_AGG_*, CPH_NUM_INT64 / CPH_NUM_FLOAT64 */
    const cph_strcol* col;                   /* a column of the build table, original row order ... */
    const void*       numbers;               /* ... or int64_t[] / double[] with one entry per row of the build table */
    int32_t           numbers_mem, reserved_;   /* CPH_MEM_HOST / CPH_MEM_DEVICE (numbers only) */
} cph_agg_spec;
typedef struct {
    uint64_t        ngroups;
    const uint64_t* first_position;          /* [ngroups] sorted position of every run's first row, ascending */
    const uint32_t* first_row;               /* [ngroups] perm[first_position[g]] */
    const uint64_t* count;                   /* [ngroups] rows per run */
    const void*     values[CPH_AGG_MAX_SPECS];   /* [nspecs] int64_t[ngroups] / double[ngroups]; the others NULL */
    int32_t         nspecs, mem;
    uint64_t        nerrors;                 /* col values that did not convert */
    uint64_t        first_error_position, first_error_row;   /* lowest such sorted position, perm[that]; UINT64_MAX */
    int32_t         first_error_kind, first_error_spec;      /* CPH_NUM_ERR_*, index into specs */
    uint64_t        host_rows;               /* float cols: values finished on the host, over all specs */
} cph_aggregated;
CPH_API int32_t cph_index_aggregate(cph_ctx* ctx, const cph_index* index, const cph_agg_spec* specs, int32_t nspecs, int32_t out_mem,
                                    cph_aggregated** out);
CPH_API void    cph_aggregated_release(cph_aggregated* a);

/*
 * Totals over a Join: one Count and up to CPH_AGG_MAX_SPECS Sum / Min / Max values per BUILD ROW of one step of a chain, on the
 * device — the reduction the reference's TestSimpleUniqueJoin (`qtyMap[id] += qty`, csvplus_test.go:368-452) and
 * TestTransformedSource (`custAmounts[cid] += amount`, csvplus_test.go:754-806) accumulate in a Go map over the JOINED stream.
 * The Join has already found the group: chain->build_row[step][m] is a dense integer below cph_index_nrows(index) for every
 * joined row m (the sorted position under CPH_CHAIN_POSITIONS, the original row id otherwise), so grouping by it needs no key
 * strings, no codec and no second index.
 *
 * A GROUP is a BUILD ROW, not a key: group g collects the joined rows with build_row[step][m] == g, ngroups ==
 * cph_index_nrows(index), and a build row no stream row matched is a group with count 0 and values 0 / +0.0.  Over an index with
 * duplicate keys every row of a run of equal keys is its own group (a stream row that matches the key joins each of them); for a
 * total per KEY the caller adds the groups of a run (cph_index_dup_groups gives the runs; with CPH_CHAIN_POSITIONS they are
 * adjacent), or joins against the unique index.
 *
 * spec.numbers holds one int64_t / double per JOINED row m (chain->nrows of them, in numbers_mem) — what cph_num_eval over the
 * joined rows returns; spec.status, when not NULL, its CPH_NUM_* byte per joined row in the same memory (cph_numcol.status).
 * The semantics are cph_index_aggregate's: an int Sum wraps as Go's `+=` does; float Min / Max are math.Min / math.Max (-0 below
 * +0, a NaN anywhere in the group gives the bits of Go's math.NaN(), also beside an infinity); a float Sum is IEEE addition in a
 * FIXED association order — the same chain and values give bit-identical sums on every call, for every out_mem and numbers_mem
 * (no floating-point atomics, nothing that depends on scheduling; the rows of a group are added in an order that is a function
 * of their row numbers alone, starting from -0.0).
 *
 * A value whose status is not 0 is DATA, not a failure: the call returns CPH_OK with nerrors > 0 (such values over all specs),
 * ngroups = 0 and every array NULL; first_error_row is the lowest such joined row m, first_error_spec the lowest spec that fails
 * there and first_error_kind its status byte.
 *
 * Tables of up to CPH_CHAIN_AGG_LDS_GROUPS groups are accumulated per workgroup in LDS and flushed once; larger ones with
 * device-scope integer atomics on the table itself, or — when a float Sum has the joined rows sorted by group anyway, or there
 * are 2^20 of them or more — over the sorted runs like the float Sum.  The results are the same either way.
 *
 * nspecs == 0 is legal (counts only), so are chain->nrows == 0 (every count 0) and an index of 1 row.  The chain may lie in host
 * or device memory, come from the fused pass or the general chain, with stream_row NULL or set (it is not read).
 * Limit: chain->nrows < 2^32.
 * CPH_ERR_INVALID (with a message): NULL ctx / chain / index / out, step outside 0..nsteps-1, chain->nrows >= 2^32, nspecs
 * outside 0..CPH_AGG_MAX_SPECS, specs NULL with nspecs > 0, an unknown op / kind / numbers_mem / out_mem, NULL numbers, a chain
 * without CPH_CHAIN_POSITIONS over an index that covers only part of its table (cph_index_select / cph_index_resolve: its row
 * ids are not dense), and an index that is not the chain step's.  A cph_chain records nothing about its indexes, so the last
 * check is by value: a build_row[step][m] that is not below cph_index_nrows(index) — an index with FEWER rows than the step's,
 * wherever the Join reached the rows it lacks.  An index with more rows cannot be told apart and gives groups of count 0.
 */
#define CPH_CHAIN_AGG_LDS_GROUPS 4096
typedef struct {
    int32_t        op, kind;         /* CPH_AGG_SUM/MIN/MAX, CPH_NUM_INT64/FLOAT64 */
    const void*    numbers;          /* int64_t[chain->nrows] / double[chain->nrows]: one value per JOINED row m */
    const uint8_t* status;           /* optional CPH_NUM_* per joined row (cph_numcol.status); NULL = all valid */
    int32_t        numbers_mem, reserved_;   /* CPH_MEM_HOST / CPH_MEM_DEVICE; `status` lies in the same mem */
} cph_chain_agg_spec;
typedef struct {
    uint64_t        ngroups;         /* == cph_index_nrows(index): one group per BUILD ROW, dense, empty groups included */
    const uint64_t* count;           /* [ngroups] joined rows whose build_row[step] == g; 0 = no stream row matched it */
    const void*     values[CPH_AGG_MAX_SPECS];  /* int64_t[ngroups] / double[ngroups]; 0 / +0.0 where count[g] == 0 */
    int32_t         nspecs, mem;
    int32_t         positions;       /* copied from the chain: g is a sorted position (1) or an original row id (0) */
    int32_t         reserved_;
    uint64_t        nerrors, first_error_row;   /* status != 0 values; lowest such joined row m, UINT64_MAX if none */
    int32_t         first_error_kind, first_error_spec;
} cph_chain_aggregated;
CPH_API int32_t cph_chain_aggregate(cph_ctx* ctx, const cph_chain* chain, int32_t step, const cph_index* index,
                                    const cph_chain_agg_spec* specs, int32_t nspecs, int32_t out_mem,
                                    cph_chain_aggregated** out);
CPH_API void    cph_chain_aggregated_release(cph_chain_aggregated* a);

/*
 * OrderBy: the rows of a selection in the order of up to CPH_ORDER_MAX_KEYS typed keys, on the device, with Drop / Top behind
 * it.  The reference has no sort by value (an Index orders by bytes, ascending only); the statement is Go's
 * slices.SortStableFunc(rows, f) where f compares key 0 first, then key 1, ...; a DESCENDING key swaps its two arguments.
 * The sort is stable: rows equal on every key keep their input order, under ascending and descending keys alike (descending
 * is not the reverse of ascending).  The answer is order[skip : skip + limit], as selection positions 0 .. nrows-1: 32-bit
 * row ids for cph_rowsel, so every writer, Map and conversion consumes an ordered list unchanged.
 *   CPH_NUM_INT64    cmp.Compare on int64.  values = int64_t[nrows] by selection position.
 *   CPH_NUM_FLOAT64  cmp.Compare on float64: a NaN is less than every non-NaN, all NaNs are equal whatever their bits,
 *                    -0 equals +0.  values = double[nrows].
 *   CPH_ORDER_BYTES  the comparison of `index` (strings.Compare per key column, csvplus.go:794-806; several key columns = the
 *                    tuple), an index built over the table being ordered: cph_index_nrows(index) == nrows and the index's
 *                    table rows are the selection positions.  Any index cph_index_aggregate accepts (32-bit, one-word and
 *                    multi-word codes, indexes out of cph_index_select / cph_index_resolve / cph_index_load).
 * Number keys lie in values_mem (a host array is uploaded); `status` (optional, same memory) holds a CPH_NUM_* byte per row, as
 * cph_col_to_number / cph_num_eval leave it, so a cph_numcol in device memory is a key without a copy.
 *
 * The keys are mapped to unsigned integers of the same order and sorted by the stable radix sort of the index build, least
 * significant key first.  With a limit, skip + limit <= nrows / 4 and option "order_select" on, the rows are first cut down
 * to the CANDIDATES: a radix select over key 0 finds the key of ascending rank skip + limit - 1, every row whose key 0 is at or
 * below it is kept in input order (all ties at the threshold included), and only those are sorted.  `select_used` tells which
 * route ran, `candidates` how many rows entered the sort (nrows without the select); the ids are the same either way.
 *
 * A row whose status is not CPH_NUM_OK is DATA, as in cph_index_aggregate: the call returns CPH_OK with nerrors > 0 (over all
 * keys), nrows = 0 and ids = NULL; first_error_row is the lowest such row, first_error_key the lowest key that fails there,
 * first_error_kind its status byte.
 *
 * nrows == 0 is legal.  More than 2^32-1 rows: CPH_ERR_TOO_MANY_ROWS.  CPH_ERR_INVALID (with a message): NULL ctx / keys / out,
 * nkeys outside 1..CPH_ORDER_MAX_KEYS, an unknown kind, values_mem or out_mem, a number key without values, a BYTES key without
 * an index or with an index of another row count.
 */
#define CPH_ORDER_MAX_KEYS 8
typedef struct {
    int32_t          kind, descending;     /* CPH_NUM_INT64 / CPH_NUM_FLOAT64 / CPH_ORDER_BYTES; 0 ascending, else descending */
    const void*      values;               /* numbers: int64_t[nrows] / double[nrows] by selection position */
    const uint8_t*   status;               /* optional CPH_NUM_* per row, same memory as values */
    int32_t          values_mem, reserved_;   /* CPH_MEM_HOST / CPH_MEM_DEVICE (numbers only) */
    const cph_index* index;                /* BYTES: an index over the table being ordered */
} cph_order_key;
typedef struct {
    uint64_t        nrows;                 /* min(limit, nrows_in - skip), 0 when skip >= nrows_in */
    const uint32_t* ids;                   /* selection positions in output order, in `mem` */
    int32_t         mem, select_used;
    uint64_t        candidates;            /* rows that entered the sort */
    uint64_t        nerrors, first_error_row;      /* lowest row with a status != OK in any key; UINT64_MAX */
    int32_t         first_error_kind, first_error_key;
} cph_ordered;
CPH_API int32_t cph_order_rows(cph_ctx* ctx, const cph_order_key* keys, int32_t nkeys, uint64_t nrows, uint64_t skip,
                               uint64_t limit /* UINT64_MAX = none */, int32_t out_mem, cph_ordered** out);
CPH_API void    cph_ordered_release(cph_ordered* o);

/* Index.WriteTo / LoadIndex (csvplus.go:655-705) for the device index: a flat
 * little-endian file with the key codec, sorted codes and perm.  NOT a gob
 * stream and without row payload: the row table stays with the caller (the
 * reference's file holds the rows because there the rows ARE the index).  A
 * short write removes the file, as the reference does (:663-671). */
CPH_API int32_t cph_index_save(cph_ctx* ctx, const cph_index* index, const char* path);
CPH_API int32_t cph_index_load(cph_ctx* ctx, const char* path, cph_index** out);

/* ---- introspection (for benchmarks / roofline accounting) -------------------- */

typedef struct {
    uint64_t nrows;
    int32_t  nkeycols;
    int32_t  key_positions;   /* total byte positions encoded (sum of per-column max length) */
    int32_t  code_words;      /* 64-bit (or one 32-bit) words per encoded key                */
    int32_t  code_bits;       /* significant bits of the most significant..least words, summed */
    int32_t  key_bytes;       /* bytes per key the sort kernels move (4 or 8)                 */
    int32_t  sort_passes;     /* radix scatter passes executed                                 */
    int32_t  direct_table;    /* 1 when the probe uses the direct-address table                */
    int32_t  dict_entries;    /* entries of the group dictionaries (0: per-position alphabets only)  */
    uint64_t table_entries;   /* entries of the direct-address table (0 if none planned)       */
    int32_t  lookup_built;    /* lookup structures BUILT so far (bits): 8 = rank table (positions), 1 = 8-byte table, 2 = 4-byte row table,
                                 4 = hash table.  direct_table / table_entries only say one is PLANNED: the
                                 structures are built by the first Join that uses them (or cph_index_prepare_join) */
    int32_t  hash_mode;       /* 0 none; 1 one code word per entry, 2 up to three words, 3 64-bit tag + verification */
    uint64_t hash_bytes;      /* size of the hash table                                                         */
    int32_t  build_path;      /* 0: general path (statistics, host codec, encode, multi-launch radix sort);
                                 1: the one-launch build of small tables (ctx option "small_build_rows", default 8192);
                                 2: host-formed codes — the key column came in host memory and only its 4-byte codes were
                                    uploaded (ctx option "host_build") */
    int32_t  split;           /* 0: none; else 0x100 * (1 + key column that is cut) + the delimiter byte: the key codec codes that
                                 column as (prefix through its first delimiter, suffix) — whole-value dictionary + per-position
                                 suffix (round 4; dict_entries then counts the prefixes) */
} cph_index_info;

CPH_API int32_t cph_index_get_info(const cph_index* index, cph_index_info* info);

/*
 * Join looks a probe row's key up in a structure that is not part of the Index (csvplus.go:612-614: the sorted rows
 * ARE the index) and is therefore built by the first Join that wants it: a direct-address table over the key codes
 * when the code space is dense (<= 24 codes per row) — for a duplicate-free index asked for sorted positions or for
 * bounds only (cph_join_chain_ex CPH_CHAIN_POSITIONS, cph_join_probe with want_pairs = 0) a RANK table instead: presence
 * bits + a running count per 32 codes, 1/16 the size of the 4-byte row table —, a hash table over the codes otherwise
 * (one 64-byte sector per probe row for any key: random ids, hashes, several columns, keys of any length); a PREFIX join (fewer columns than
 * the index has, csvplus.go:546-550) needs the order and searches the sorted codes, as does every Join when the
 * structure cannot be allocated.  This call builds the structure NOW — `chained` = 1: the one cph_join_chain /
 * cph_stream_join use (4-byte row table for a duplicate-free index), 2: the one cph_join_chain_ex uses with
 * CPH_CHAIN_POSITIONS (the rank table), 0: the one cph_join_probe uses for pairs — so that
 * the first Join does not pay for it.
 *
 * Sharing an index between ctxs: the structures are built on the INDEX's ctx (its stream, its pool) whatever ctx
 * runs the Join, and a Join on another ctx of the same device orders its stream behind that build.  Two threads
 * with a ctx each may join against one index at the same time: the lazy build is serialised per index and the
 * index ctx's device pool is locked (since round 4; cph_index_prepare_join remains the way to keep the build out
 * of the first Join).  The index's OWN ctx must not be destroyed — nor the index itself — while another thread joins
 * against it.
 */
CPH_API int32_t cph_index_prepare_join(cph_index* index, int32_t chained);

/*
 * Per-kernel timing for roofline accounting.  While enabled, every kernel launch
 * of this ctx is bracketed by two HIP events on the ctx's stream.
 * cph_ctx_profile_read synchronises the stream and returns, per kernel name, the
 * number of launches, their summed duration and their summed ALGORITHMIC bytes
 * (the per-launch byte model documented in DESIGN.md; 0 where the library cannot
 * know the input's value bytes).  *n receives the number of distinct kernels
 * (may exceed cap).  reset != 0 clears the statistics afterwards.
 */
typedef struct {
    char     name[48];
    uint64_t launches;
    double   total_ms;
    double   algo_bytes;
} cph_kernel_stat;

CPH_API int32_t cph_ctx_profile(cph_ctx* ctx, int32_t enable);
/* The two events around a launch cost ~10 us of stream time each: a loop of many short kernels measurably slows
 * down under cph_ctx_profile.  This variant times ONLY the launches of `kernel_name` (NULL: profiling off), so a
 * benchmark can time its dominant kernel inside the timed region without disturbing the region. */
CPH_API int32_t cph_ctx_profile_only(cph_ctx* ctx, const char* kernel_name);
CPH_API int32_t cph_ctx_profile_read(cph_ctx* ctx, cph_kernel_stat* out, int32_t cap, int32_t* n, int32_t reset);

/*
 * What this box's memory system sustains for the two access patterns the Join kernels are made of (a measurement
 * utility, not part of the hot path): kind 0 = streaming copy, `bytes` read + `bytes` written with 16 bytes per lane;
 * kind 1 = random gather of 4-byte entries, `n` lookups into a table of `bytes` bytes, 4 lookups in flight per thread,
 * the indices (4 B) streamed in and the values (4 B) streamed out — one direct-table step of the chained-join kernel
 * without any key decoding.  *ms = average of `reps` launches after two warm-up launches (HIP events on the ctx stream).
 */
CPH_API int32_t cph_calibrate(cph_ctx* ctx, int32_t kind, uint64_t bytes, uint64_t n, int32_t reps, double* ms);

/* Library version, e.g. "csvplus_hip 0.1 (gfx950)". */
CPH_API const char* cph_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSVPLUS_HIP_H */
