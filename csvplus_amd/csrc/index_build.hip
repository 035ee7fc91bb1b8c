// index_build.hip — the host side of IndexOn / UniqueIndexOn (csvplus.go:529-537, 707-756): what cph_index_build and
// cph_index_build_many (capi.hip) run between their argument checks and their return codes.
//
// One index build in three phases, so that a batch of builds shares its two host round trips:
// (1) stage the columns, enqueue the alphabet statistics  | sync 1: statistics of every index |
// (2) codec on the host, encode + sort + adjacent-equal scan enqueued  | sync 2: first duplicate of every index |
// (3) table decision.
// In a two-stream batch sync 1 is taken per stream: the jobs of the main stream run their phase 2 as soon as that stream has
// delivered, the side stream's jobs behind its own synchronisation (sync1_then_phase2).
#include <algorithm>
#include <new>

#include "cph_internal.hpp"
#include "codec_device.hpp"

namespace cph {

// ---- what both the device-coded and the host-coded (host_encode.hip) build end in ------------------------------

void index_set_sorted(cph_index* ix, DevBuf&& codes, DevBuf&& perm, int passes) {
    ix->sorted_codes = std::move(codes);
    ix->perm = std::move(perm);
    ix->sort_passes = passes;
}

// ... after radix_sort_pairs, which leaves its result in either buffer of each pair
template <class K>
static void index_set_sorted(cph_index* ix, const K* kout, DevBuf& ka, DevBuf& kb, const uint32_t* vout, DevBuf& va, DevBuf& vb, int passes) {
    index_set_sorted(ix, std::move(kout == ka.as<K>() ? ka : kb), std::move(vout == va.as<uint32_t>() ? va : vb), passes);
}

void index_reset_for_rebuild(cph_index* ix) {
    ix->codec = CodecHost{};
    ix->codec_dev.reset(); ix->sorted_codes.reset(); ix->perm.reset(); ix->first_dup_dev.reset(); ix->ranktab.reset();
}

bool direct_sort_applies(const cph_ctx* ctx, bool unique, uint64_t n, uint64_t states) {
    return unique && ctx->direct_sort != 0 && n >= (1ull << 16) && states >= n && states <= 2 * n && states < 0xFFFFFFFFull;
}

// The classic radix passes over one 32-bit code word that may hold duplicates: sorts `codes` (destroyed) through kb / va and a
// fourth buffer of its own, publishes the result, runs and reads the adjacent-equal scan, plans the table.
// ctx->stream: synchronised on return.
Status sort_codes_classic(cph_ctx* ctx, cph_index* ix, DevBuf& codes, DevBuf& kb, DevBuf& va) {
    const uint64_t n = ix->nrows;
    DevBuf vb;
    CPH_TRY(vb.alloc(&ctx->pool, n * sizeof(uint32_t)));
    uint32_t *kout = nullptr, *vout = nullptr;
    int passes = 0;
    CPH_TRY(radix_sort_pairs<uint32_t>(ctx, codes.as<uint32_t>(), kb.as<uint32_t>(), va.as<uint32_t>(), vb.as<uint32_t>(), true, n,
                                       ix->codec.word_bits[0], &kout, &vout, &passes));
    index_set_sorted(ix, kout, codes, kb, vout, va, vb, passes);
    CPH_TRY(index_first_dup_launch(ctx, ix));
    CPH_TRY(index_first_dup_read(ctx, ix));
    index_plan_table(ix);
    return {};
}

// A counted window sort (counted_sort.hip) reported a window beyond its capacity through *over: nothing was sorted, `codes` are
// untouched, kb / va are the buffers it would have filled.  The rows cluster (a dense block in a sparse code space: the plan went
// by the average): up to `narrower_attempts` times windows a quarter as wide as before, then the classic passes — a retry costs
// the histogram + one wait (0.1 ms per 1e8 rows), the classic sort 2 ms.
// ctx->stream: idle on entry, synchronised on return.
Status sort_codes_after_overflow(cph_ctx* ctx, cph_index* ix, DevBuf& codes, DevBuf& kb, DevBuf& va, uint32_t* over, int narrower_attempts) {
    const uint64_t n = ix->nrows, states = ix->codec.word_states[0];
    ix->first_dup_dev.reset();
    CountedSortPlan first;
    int wb = narrower_attempts > 0 && counted_sort_plan(ctx, n, states, &first) ? (int)first.wbits : 0;
    for (int attempt = 0; attempt < narrower_attempts && wb > 0; attempt++) {
        wb -= 2;
        CountedSortPlan csp;
        if (!counted_sort_plan(ctx, n, states, &csp, wb) || (int)csp.wbits != wb) break;
        CPH_TRY(ix->first_dup_dev.alloc(&ctx->pool, sizeof(uint32_t)));
        CPH_TRY(counted_sort(ctx, csp, codes.as<uint32_t>(), n, states, va.as<uint32_t>(), kb.as<uint32_t>(), ix->first_dup_dev.as<uint32_t>(), over));
        CPH_HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (*(volatile uint32_t*)over == 0) {
            index_set_sorted(ix, std::move(kb), std::move(va), 0);
            CPH_TRY(index_first_dup_read(ctx, ix));
            index_plan_table(ix);
            return {};
        }
        ix->first_dup_dev.reset();
    }
    return sort_codes_classic(ctx, ix, codes, kb, va);
}

// ---- one build job and what its current attempt may try --------------------------------------------------------

// Where the attempt's alphabets come from.  A first attempt picks its source in build_phase1; a restarted one is
// given SplitExact or ExactStats (restart_job) — a restart never samples and never takes the one-launch path.
enum class Alphabets : uint8_t {
    OneLaunch,         // small table: statistics, codec, sort and scan inside k_small_build (small_build.hip) — no phase 2, no sync 2
    SplitFromSample,   // delimiter-split codec built from a SAMPLE alone (codec_try_split, speculative) before any statistics pass
    SplitExact,        // the same codec from the exact split statistics
    Sample,            // alphabets from a sample of the rows (keycodec.hip: codec_sample_*)
    ExactStats,        // the statistics pass over all rows (codec_stats_launch)
};
// Under SplitFromSample, SplitExact, Sample — and under ExactStats when phase 2 picks a split codec or the direct sort — the
// kernels check every row and raise BuildJob::miss for one they cannot handle.  What follows, all of it in next_attempt:
//
//   the attempt that failed                  | the next attempt                          | may not try again
//   -----------------------------------------+-------------------------------------------+-------------------
//   OneLaunch, key "not small"               | ExactStats                                | —
//   SplitFromSample, miss                    | SplitExact (ctx->n_split_respec++), or    | direct
//                                            | ExactStats when the exact statistics want |
//                                            | no split after all                        |
//   SplitExact, miss                         | ExactStats                                | split, direct
//   Sample, miss or direct-sort duplicate    | ExactStats (the general sort says WHERE)  | split, direct
//   ExactStats, the same two                 | ExactStats                                | split, direct
//
// A counted-sort overflow is no restart: the same codes are sorted again (sort_codes_after_overflow).
struct Avoid {
    bool split = false;    // no delimiter-split codec (build_phase2)
    bool direct = false;   // no optimistic direct sort (build_encode_sort)
};

struct BuildJob {
    cph_index* ix = nullptr;
    int32_t nkeycols = 0;
    std::vector<DevBuf> staged;
    DevCol dcols[kMaxKeyCols];
    DevBuf stats_dev;
    const void* sample_host = nullptr;   // Sample: where the sample kernel itself leaves its result (report words of the ctx: no read-back copy)
    size_t scratch_off = 0;      // where this job's read-backs land in the batch's read-back block
    GroupSpec spec;              // speculative dictionaries (codec_try_groups)
    Alphabets from = Alphabets::ExactStats;
    Avoid avoid;
    SmallBufs sbufs;             // OneLaunch
    bool unique = false;         // the caller expects distinct keys (UniqueIndexOn): the optimistic direct sort may be tried
    bool side = false;           // this job's work is enqueued on the ctx's side stream (build_indexes: it overlaps its neighbour's)
    uint32_t* miss = nullptr;    // report word (pinned host memory, host_word) raised by the encode kernel of a split / sampled codec and by the
                                 // optimistic direct sort; read after the build's last synchronisation
    uint32_t* cs_over = nullptr; // counted window sort (counted_sort.hip): report word raised when a window does not fit — nothing was sorted then,
    DevBuf cs_codes;             // ... and the classic passes run over these (untouched) codes after the build's last synchronisation

    bool one_launch() const { return from == Alphabets::OneLaunch; }
    bool presplit() const { return from == Alphabets::SplitFromSample || from == Alphabets::SplitExact; }
    bool sampled() const { return from == Alphabets::Sample; }
    // what sync 1 brings to the host for this job (a sample's result is written to the host by its kernel)
    size_t readback_bytes() const { return one_launch() ? sizeof(SmallResult) : (presplit() || sampled()) ? 0 : sizeof(ColStats) * (size_t)nkeycols; }
};

struct NextAttempt {
    Alphabets from;
    Avoid avoid;
};
// The one place that says what follows a failed attempt (the table above).  `j` is the job as the failed attempt left it.
static NextAttempt next_attempt(const BuildJob& j) {
    switch (j.from) {
    case Alphabets::OneLaunch: return {Alphabets::ExactStats, {}};
    case Alphabets::SplitFromSample: return {Alphabets::SplitExact, {false, true}};
    case Alphabets::SplitExact:
    case Alphabets::Sample:
    case Alphabets::ExactStats: break;
    }
    return {Alphabets::ExactStats, {true, true}};
}

static Status build_phase1(cph_ctx* ctx, const cph_strcol* keycols, int32_t nkeycols, BuildJob* job) {
    CPH_TRY(validate_cols(keycols, nkeycols));
    cph_index* ix = job->ix;
    ix->ctx = ctx;
    ix->nrows = keycols[0].nrows;
    ix->table_rows = ix->nrows;
    ix->nkeycols = nkeycols;
    job->nkeycols = nkeycols;
    CPH_TRY(stage_cols(ctx, keycols, nkeycols, &job->staged, job->dcols));
    if (small_build_applies(ctx, job->dcols, nkeycols, ix->nrows)) {   // launched by enqueue_readbacks (needs its result slot)
        job->from = Alphabets::OneLaunch;
        return {};
    }
    // "sample first": a large table over ONE variable-length key column asks a sample whether its keys want the delimiter split
    // (keycodec.hip); when they do, the split codec is there BEFORE any plain statistics (one read of the strings less)
    if (nkeycols == 1 && !job->dcols[0].fixed_width && ix->nrows >= (1ull << 22)) {
        bool from_sample = false;
        CPH_TRY(codec_try_split(ctx, job->dcols, 1, ix->nrows, nullptr, &ix->codec, true, &from_sample));
        if (ix->codec.has_split()) {
            job->from = from_sample ? Alphabets::SplitFromSample : Alphabets::SplitExact;
            return {};
        }
    }
    if (codec_sample_applies(ctx, job->dcols, nkeycols, ix->nrows)) {
        job->from = Alphabets::Sample;
        return codec_sample_launch(ctx, job->dcols[0], ix->nrows, &job->sample_host);
    }
    job->from = Alphabets::ExactStats;
    return codec_stats_launch(ctx, job->dcols, nkeycols, &job->stats_dev);   // K0: alphabets
}

static Status job_arm_miss(cph_ctx* ctx, BuildJob* job) {
    job->miss = host_word(ctx);
    return job->miss ? Status{} : Status{CPH_ERR_HIP, "no pinned host memory for the report words of a build"};
}

// Stable LSD sort over `nw` 64-bit code words per row (all[w][n], word 0 most significant; bits[w] significant
// bits each): least significant word first, the later words gathered through the permutation so far.  Leaves the
// sorted words (word-major) and the permutation in the index.
static Status sort_words_lsd(cph_ctx* ctx, cph_index* ix, const uint64_t* all, int nw, const int* bits, uint64_t n, DevBuf& va,
                             DevBuf& vb) {
    DevBuf ka, kb;
    CPH_TRY(ka.alloc(&ctx->pool, n * sizeof(uint64_t)));
    CPH_TRY(kb.alloc(&ctx->pool, n * sizeof(uint64_t)));
    uint32_t* vcur = va.as<uint32_t>();
    uint32_t* vother = vb.as<uint32_t>();
    uint64_t* kout = ka.as<uint64_t>();
    bool first = true;
    int passes = 0, total_passes = 0;
    for (int w = nw - 1; w >= 0; w--) {
        const uint64_t* word = all + (uint64_t)w * n;
        if (first) {
            if (n) CPH_HIP_TRY(hipMemcpyAsync(ka.get(), word, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            CPH_TRY(gather_u64(ctx, word, vcur, ka.as<uint64_t>(), n));
        }
        uint32_t* vout;
        CPH_TRY(radix_sort_pairs<uint64_t>(ctx, ka.as<uint64_t>(), kb.as<uint64_t>(), vcur, vother, first, n, bits[w], &kout, &vout,
                                           &passes));
        total_passes += passes;
        if (vout != vcur) { vother = vcur; vcur = vout; }
        first = false;
    }
    // sorted codes, word-major: word 0 is the key output of the last sort (a streaming copy);
    // only the less significant words need a gather through the final permutation
    DevBuf sorted;
    CPH_TRY(sorted.alloc(&ctx->pool, (size_t)nw * n * sizeof(uint64_t)));
    if (n) CPH_HIP_TRY(hipMemcpyAsync(sorted.get(), kout, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
    for (int w = 1; w < nw; w++) CPH_TRY(gather_u64(ctx, all + (uint64_t)w * n, vcur, sorted.as<uint64_t>() + (uint64_t)w * n, n));
    index_set_sorted(ix, std::move(sorted), std::move(vcur == va.as<uint32_t>() ? va : vb), total_passes);
    return {};
}

// Segment view of a staged key column for one window.
static DevCol window_col(const DevCol* cols, const cph_key_window& w, int s) {
    DevCol v = cols[w.seg_col[s]];
    v.skip = w.seg_skip[s];
    v.take = w.seg_take[s];
    return v;
}

// Keys whose columns need more than kMaxKeyBytes byte positions: the positions (column-major) are cut into windows
// of at most kMaxKeyBytes, every window gets its own codec over its column segments, and the rows are sorted LSD
// over all the windows' words — the order Less (csvplus.go:794-807) defines has no length limit, only the tuned
// single-window paths do.
static Status build_multi_window(cph_ctx* ctx, BuildJob* job, const std::vector<ColStats>& raw) {
    cph_index* ix = job->ix;
    const uint64_t n = ix->nrows;
    std::vector<cph_key_window>& W = ix->windows;
    W.clear();
    W.emplace_back();
    uint32_t room = kMaxKeyBytes;
    for (int c = 0; c < job->nkeycols; c++) {
        uint32_t left = raw[(size_t)c].maxlen, skip = 0;
        do {
            if (room == 0 || W.back().nseg == kMaxKeyCols) {
                W.emplace_back();
                room = kMaxKeyBytes;
            }
            cph_key_window& w = W.back();
            const uint32_t t = left < room ? left : room;
            w.seg_col[w.nseg] = c;
            w.seg_skip[w.nseg] = skip;
            w.seg_take[w.nseg] = t == left ? 0xFFFFFFFFu : t;   // the column's last segment runs to the end of the value
            w.nseg++;
            skip += t;
            left -= t;
            room -= t;
        } while (left > 0);
    }
    int total_words = 0;
    for (auto& w : W) {
        DevCol v[kMaxKeyCols];
        for (int s = 0; s < w.nseg; s++) v[s] = window_col(job->dcols, w, s);
        std::vector<ColStats> st;
        CPH_TRY(codec_collect_stats(ctx, v, w.nseg, &st));
        CPH_TRY(codec_build(st, &w.codec));
        w.codec.key32 = false;   // window words are always stored as 64-bit words
        CPH_TRY(codec_upload(ctx, w.codec, &w.codec_dev));
        w.word_base = total_words;
        total_words += w.codec.nwords;
    }
    ix->codec = W[0].codec;
    DevBuf all, va, vb;
    CPH_TRY(all.alloc(&ctx->pool, (size_t)total_words * n * sizeof(uint64_t)));
    CPH_TRY(va.alloc(&ctx->pool, n * sizeof(uint32_t)));
    CPH_TRY(vb.alloc(&ctx->pool, n * sizeof(uint32_t)));
    std::vector<int> bits((size_t)total_words);
    for (auto& w : W) {
        DevCol v[kMaxKeyCols];
        for (int s = 0; s < w.nseg; s++) v[s] = window_col(job->dcols, w, s);
        CPH_TRY(codec_encode_build(ctx, w.codec, w.codec_dev, v, n, all.as<uint64_t>() + (uint64_t)w.word_base * n));
        for (int k = 0; k < w.codec.nwords; k++) bits[(size_t)(w.word_base + k)] = w.codec.word_bits[k];
    }
    CPH_TRY(sort_words_lsd(ctx, ix, all.as<uint64_t>(), total_words, bits.data(), n, va, vb));
    return index_first_dup_launch(ctx, ix);
}

static Status build_encode_sort(cph_ctx* ctx, BuildJob* job);

// The job's statistics are on the host (stats_host; none for a presplit job): codec, then encode + sort + scan enqueued.
static Status build_phase2(cph_ctx* ctx, BuildJob* job, const void* stats_host) {
    cph_index* ix = job->ix;
    const uint64_t n = ix->nrows;
    const int32_t nkeycols = job->nkeycols;
    const DevCol* dcols = job->dcols;
    if (job->presplit()) {   // the codec is there already (build_phase1, restart_job)
        CPH_TRY(job_arm_miss(ctx, job));
        CPH_TRY(codec_upload(ctx, ix->codec, &ix->codec_dev));
        return build_encode_sort(ctx, job);
    }
    std::vector<ColStats> stats;
    if (job->sampled()) {
        codec_sample_finish(dcols[0], stats_host, &stats);
        CPH_TRY(codec_build(stats, &ix->codec));
        if (codec_sample_checked(ix->codec, dcols)) {
            CPH_TRY(job_arm_miss(ctx, job));
            CPH_TRY(codec_upload(ctx, ix->codec, &ix->codec_dev));
            return build_encode_sort(ctx, job);
        }
        // a code the checking encode kernel does not handle (several words, ...): the exact pass after all, here and now
        job->from = Alphabets::ExactStats;
        ix->codec = CodecHost{};
        CPH_TRY(codec_collect_stats(ctx, dcols, nkeycols, &stats));
    } else {
        codec_stats_finish(dcols, nkeycols, stats_host, &stats);
    }
    uint64_t positions = 0;
    for (const auto& s : stats) positions += s.maxlen;
    if (positions > (uint64_t)kMaxKeyBytes) return build_multi_window(ctx, job, stats);
    CPH_TRY(codec_build(stats, &ix->codec));
    if (!job->avoid.split) CPH_TRY(codec_try_split(ctx, dcols, nkeycols, n, &stats, &ix->codec));   // only acts on codes beyond 32 bits
    if (ix->codec.has_split()) {
        CPH_TRY(job_arm_miss(ctx, job));
    } else {
        CPH_TRY(codec_try_groups(ctx, dcols, nkeycols, n, &ix->codec, &job->spec));   // only acts on codes of several words
    }
    CPH_TRY(codec_upload(ctx, ix->codec, &ix->codec_dev));
    return build_encode_sort(ctx, job);
}

// The classic passes over the single-word codes in ka (32- or 64-bit), the first histogram already in eh when the encode kernel left it.
template <class K>
static Status sort_single_word(cph_ctx* ctx, cph_index* ix, DevBuf& ka, DevBuf& kb, DevBuf& va, DevBuf& vb, const EncodeHist& eh) {
    K* kout;
    uint32_t* vout;
    int passes = 0;
    CPH_TRY(radix_sort_pairs<K>(ctx, ka.as<K>(), kb.as<K>(), va.as<uint32_t>(), vb.as<uint32_t>(), true, ix->nrows, ix->codec.word_bits[0], &kout,
                                &vout, &passes, eh.counts, eh.done));
    index_set_sorted(ix, kout, ka, kb, vout, va, vb, passes);
    return {};
}

// Encode with the index's codec, sort, launch the adjacent-equal scan.
static Status build_encode_sort(cph_ctx* ctx, BuildJob* job) {
    cph_index* ix = job->ix;
    const uint64_t n = ix->nrows;
    const DevCol* dcols = job->dcols;
    const CodecHost& cd = ix->codec;

    DevBuf va, vb;
    CPH_TRY(va.alloc(&ctx->pool, n * sizeof(uint32_t)));

    if (cd.nwords == 1) {
        // single-word codes: the encode kernel leaves the first radix pass's histogram behind when it can
        const size_t kb_ = cd.key32 ? sizeof(uint32_t) : sizeof(uint64_t);
        DevBuf ka, kb, counts;
        CPH_TRY(ka.alloc(&ctx->pool, n * kb_));
        EncodeHist eh;
        // distinct keys expected over a dense code space: slot[code] = row instead of radix passes (window_sort.hip)
        const uint64_t states = cd.word_states[0];
        const bool direct = !job->avoid.direct && cd.key32 && !job->spec.active && direct_sort_applies(ctx, job->unique, n, states);
        if (direct) {   // (writes va and ka alone: the second pair of buffers is not allocated)
            if (!job->miss) {
                CPH_TRY(job_arm_miss(ctx, job));
            }
            // fixed-width 8-byte keys under an arithmetic codec (decimal ids): the first partition level of the window sort codes the keys
            // itself — no encode kernel, no code array written and read again
            // a code space larger than the table: the Join's rank table (8 bytes per 32 codes) falls out of the window sort for free
            DevBuf rt;
            uint64_t rt_blocks = 0;
            if (ctx->direct_ranktab && ctx->direct_sort == 1 && states != n && states <= (1ull << 30)) {   // (index_plan_table's limit)
                rt_blocks = ranktab_blocks(states);
                if (!rt.alloc(&ctx->pool, rt_blocks * 8).ok()) rt_blocks = 0;   // (then the first Join builds it, or does without)
            }
            void* rtp = rt_blocks ? rt.get() : nullptr;
            ArithPlan ap;
            codec_arith_plan(cd, &ap);
            const DevCol& kc = dcols[0];
            if (ctx->direct_sort == 1 && ctx->direct_fused_encode && job->nkeycols == 1 && ap.enabled && ap.keylen == 8 && kc.fixed_width == 8 &&
                !kc.segmented() && ((uintptr_t)kc.data & 15) == 0) {
                CPH_TRY(direct_sort_windows_keys(ctx, reinterpret_cast<const uint64_t*>(kc.data), ap, n, states, va.as<uint32_t>(), ka.as<uint32_t>(),
                                                 job->miss, rtp, rt_blocks));
            } else {
                CPH_TRY(codec_encode_build(ctx, cd, ix->codec_dev, dcols, n, ka.get(), &eh, nullptr, job->miss));
                CPH_TRY(direct_sort_windows(ctx, ka.as<uint32_t>(), n, states, va.as<uint32_t>(), ka.as<uint32_t>(), job->miss, rtp, rt_blocks));
            }
            if (rtp) ix->ranktab = std::move(rt);   // (a miss starts the build over and drops it: restart_job)
            index_set_sorted(ix, std::move(ka), std::move(va), 0);
            // no adjacent-equal scan (first_dup_dev stays empty): either the keys are distinct or the miss word sends the build down the general path
            return {};
        }
        // duplicates allowed, 32-bit codes, a window of the code space holds a few thousand rows: MSD sort through counted LDS windows
        // (counted_sort.hip) instead of 3-4 classic passes; the adjacent-equal scan falls out of it
        CPH_TRY(kb.alloc(&ctx->pool, n * kb_));
        CountedSortPlan csp;
        if (cd.key32 && !job->spec.active && counted_sort_plan(ctx, n, states, &csp)) {
            uint32_t* over = host_word(ctx);
            if (!over) return {CPH_ERR_HIP, "no pinned host memory for the report words of a build"};
            CountedSort cs;
            CPH_TRY(cs.begin(ctx, csp, n));
            CPH_TRY(codec_encode_build(ctx, cd, ix->codec_dev, dcols, n, ka.get(), &eh, &job->spec, job->miss));
            CPH_TRY(ix->first_dup_dev.alloc(&ctx->pool, sizeof(uint32_t)));
            CPH_TRY(cs.run(ctx, ka.as<uint32_t>(), n, states, va.as<uint32_t>(), kb.as<uint32_t>(), ix->first_dup_dev.as<uint32_t>(), over, false));
            job->cs_over = over;
            job->cs_codes = std::move(ka);
            index_set_sorted(ix, std::move(kb), std::move(va), 0);
            return {};
        }
        CPH_TRY(vb.alloc(&ctx->pool, n * sizeof(uint32_t)));
        const RadixPlan plan = radix_plan(ctx, n, cd.word_bits[0]);
        if (plan.npass > 0) {
            CPH_TRY(counts.alloc(&ctx->pool, plan.count_words() * sizeof(uint32_t)));
            eh.tile_rows = plan.tile;
            eh.digit_mask = (1u << plan.nb0) - 1u;
            eh.bins = 1u << plan.rbits;
            eh.counts = counts.as<uint32_t>();
        }
        CPH_TRY(codec_encode_build(ctx, cd, ix->codec_dev, dcols, n, ka.get(), &eh, &job->spec, job->miss));
        if (job->spec.active) {
            // speculative dictionaries (from a sample of the rows): did the encode kernel meet a window they lack?  Then
            // it has added every such window to the device sets: rebuild the codec from the now complete sets and encode
            // again.  (One more synchronisation, in exchange for the exact statistics pass over all rows.)
            uint32_t miss = 0;
            CPH_TRY(read_device_value(ctx, job->spec.miss.as<uint32_t>(), &miss));
            job->spec.active = false;
            if (miss) {
                const int bits_before = cd.word_bits[0];
                CPH_TRY(codec_groups_complete(ctx, dcols, job->nkeycols, n, miss, &job->spec, &ix->codec));
                CPH_TRY(codec_upload(ctx, ix->codec, &ix->codec_dev));
                // the same single-word shape (the usual outcome: a few more dictionary entries): encode into the same
                // buffers; anything else starts over with the new codec
                if (cd.nwords != 1 || cd.word_bits[0] != bits_before || radix_plan(ctx, n, cd.word_bits[0]).npass != plan.npass) {
                    ka.reset(); kb.reset(); counts.reset(); va.reset(); vb.reset();
                    return build_encode_sort(ctx, job);
                }
                CPH_TRY(codec_encode_build(ctx, cd, ix->codec_dev, dcols, n, ka.get(), &eh, nullptr));
            }
        }
        if (cd.key32) CPH_TRY(sort_single_word<uint32_t>(ctx, ix, ka, kb, va, vb, eh));
        else CPH_TRY(sort_single_word<uint64_t>(ctx, ix, ka, kb, va, vb, eh));
    } else {
        // multi-word codes: LSD over the words, least significant word first
        DevBuf all;
        CPH_TRY(vb.alloc(&ctx->pool, n * sizeof(uint32_t)));
        CPH_TRY(all.alloc(&ctx->pool, (size_t)cd.nwords * n * sizeof(uint64_t)));
        CPH_TRY(codec_encode_build(ctx, cd, ix->codec_dev, dcols, n, all.get(), nullptr, nullptr, job->miss));
        CPH_TRY(sort_words_lsd(ctx, ix, all.as<uint64_t>(), cd.nwords, cd.word_bits, n, va, vb));
    }

    // adjacent-equal scan; its result is read back by sync2_and_read together with the other jobs'
    CPH_TRY(index_first_dup_launch(ctx, ix));
    return {};
}

// ---- a batch of jobs from phase 1 to its indexes ---------------------------------------------------------------

struct Batch {
    cph_ctx* ctx;
    std::vector<BuildJob>& jobs;
    std::vector<Status>& status;   // status[i].ok() on entry: phase 1 of job i succeeded; on exit: the job's outcome
    bool any_side = false;         // some job runs on the side stream
    bool any_general = false;      // some job goes through phase 2 and sync 2
    // Two streams: phase 2 of the main stream's jobs runs while the side stream's read-backs are still on their way, and phase 2
    // may use (and grow) ctx->pinned_scratch — the batch's read-backs then land in a block of their own, held until the batch ends.
    struct ReadbackBlock {
        cph_ctx* c;
        void* p = nullptr;
        size_t cap = 0;
        bool settled = false;   // every stream that writes into the block has been synchronised
        // (a return in between, after a failed synchronisation: copies may still be on their way — the block is not handed on)
        ~ReadbackBlock() { if (settled) pinned_cache_put(c, p, cap); }
    } rb;
    uint8_t* h = nullptr;          // where sync 1's read-backs land (job i at h + jobs[i].scratch_off)
    std::vector<size_t> not_small;    // one-launch candidates whose key needs the general path after all
    std::vector<size_t> missed;       // jobs whose kernels met a row they could not handle (BuildJob::miss)
    std::vector<size_t> overflowed;   // jobs whose counted window sort met a window beyond its capacity
    Batch(cph_ctx* c, std::vector<BuildJob>& j, std::vector<Status>& s) : ctx(c), jobs(j), status(s), rb{c} {}
};

// Lays out the read-backs of sync 1, launches the one-launch builds (they write their result slot themselves) and enqueues the
// statistics copies, each on its job's stream.  Streams: busy with phase 1 on entry, nothing is waited for.
static Status enqueue_readbacks(Batch& b) {
    cph_ctx* ctx = b.ctx;
    size_t total = 0;
    for (size_t i = 0; i < b.jobs.size(); i++) {
        BuildJob& j = b.jobs[i];
        j.scratch_off = total;
        total += j.readback_bytes();
        total = (total + 63) & ~(size_t)63;
        if (b.status[i].ok() && !j.one_launch()) b.any_general = true;
        b.any_side = b.any_side || j.side;
    }
    if (total < 64) total = 64;
    CPH_TRY(b.any_side ? pinned_cache_get(ctx, result_block_bytes(total), &b.rb.p, &b.rb.cap) : ensure_pinned_scratch(ctx, total));
    b.h = static_cast<uint8_t*>(b.any_side ? b.rb.p : ctx->pinned_scratch);
    for (size_t i = 0; i < b.jobs.size(); i++) {
        BuildJob& j = b.jobs[i];
        if (!b.status[i].ok()) continue;
        if (j.one_launch()) {
            SideStream on_side(ctx, j.side);   // (its columns were staged on that stream)
            b.status[i] = small_build_launch(ctx, j.dcols, j.nkeycols, j.ix->nrows, &j.sbufs, reinterpret_cast<SmallResult*>(b.h + j.scratch_off));
            continue;
        }
        if (!j.readback_bytes()) continue;
        hipError_t e = hipMemcpyAsync(b.h + j.scratch_off, j.stats_dev.get(), j.readback_bytes(), hipMemcpyDeviceToHost,
                                      j.side ? ctx->side_stream : ctx->stream);
        if (e != hipSuccess) b.status[i] = {CPH_ERR_HIP, std::string("statistics read-back: ") + hipGetErrorString(e)};
    }
    return {};
}

// Sync 1, per stream: a job's phase 2 needs what ITS stream brought to the host and nothing of the other's, so the main stream's
// jobs are on their way again before the host waits for the side stream (and a read-back is consumed only behind the
// synchronisation of the stream that carries it).  One-launch builds are complete here.
// Streams: busy on entry; on exit each has been synchronised once and carries its jobs' phase 2.
static Status sync1_then_phase2(Batch& b) {
    cph_ctx* ctx = b.ctx;
    const size_t nj = b.jobs.size();
    std::vector<std::vector<uint8_t>> stats_host(nj);
    for (int on = 0; on < (b.any_side ? 2 : 1); on++) {
        if (hipStreamSynchronize(on ? ctx->side_stream : ctx->stream) != hipSuccess) return {CPH_ERR_HIP, "hipStreamSynchronize failed"};
        // One stream: it is idle, parked blocks may change hands.  Two: there is no moment between the phases at which both are
        // idle any more (the main stream's phase 2 is enqueued while the side stream still runs its phase 1), so the blocks
        // parked so far wait for the flush behind sync 2.
        if (!b.any_side) ctx->pool.flush_deferred();
        // the host copies must survive phase 2 (which may reuse the scratch): take them out
        for (size_t i = 0; i < nj; i++) {
            BuildJob& j = b.jobs[i];
            if (!b.status[i].ok() || j.side != (on != 0)) continue;
            if (j.one_launch()) {
                const SmallResult res = *reinterpret_cast<const SmallResult*>(b.h + j.scratch_off);
                bool not_small = false;
                b.status[i] = small_build_finish(ctx, j.ix, j.nkeycols, &j.sbufs, &res, &not_small);
                j.sbufs = SmallBufs{};
                if (b.status[i].ok() && not_small) b.not_small.push_back(i);
                else if (b.status[i].ok()) index_plan_table(j.ix);
            } else if (j.sampled()) {
                const uint8_t* sh = static_cast<const uint8_t*>(j.sample_host);
                stats_host[i].assign(sh, sh + codec_sample_bytes());
            } else if (!j.presplit()) {
                stats_host[i].assign(b.h + j.scratch_off, b.h + j.scratch_off + j.readback_bytes());
            }
        }
        for (size_t i = 0; i < nj; i++) {
            BuildJob& j = b.jobs[i];
            if (!b.status[i].ok() || j.one_launch() || j.side != (on != 0)) continue;
            SideStream on_side(ctx, j.side);
            b.status[i] = build_phase2(ctx, &j, stats_host[i].data());
        }
    }
    b.rb.settled = true;
    std::sort(b.not_small.begin(), b.not_small.end());   // (the order in which the small builds are tried again stays the jobs' order)
    return {};
}

// Sync 2: the first duplicate of every job that went through phase 2, and its two report words — a miss puts the job on
// b.missed, a counted-sort overflow on b.overflowed; every other job is complete (table planned).
// Streams: busy with phase 2 on entry, both idle on exit (parked pool blocks have changed hands).
static Status sync2_and_read(Batch& b) {
    cph_ctx* ctx = b.ctx;
    const size_t nj = b.jobs.size();
    if (!b.any_general) return {};
    CPH_TRY(ensure_pinned_scratch(ctx, 2 * sizeof(uint32_t) * nj + 64));
    uint32_t* fd = static_cast<uint32_t*>(ctx->pinned_scratch);
    for (size_t i = 0; i < nj; i++) {
        BuildJob& j = b.jobs[i];
        if (!b.status[i].ok() || j.one_launch()) continue;
        fd[i] = 0xFFFFFFFFu;   // no adjacent-equal scan ran (the direct sort): distinct keys, or the miss word sends the build round again
        if (!j.ix->first_dup_dev) continue;
        hipError_t e = hipMemcpyAsync(&fd[i], j.ix->first_dup_dev.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, j.side ? ctx->side_stream : ctx->stream);
        if (e != hipSuccess) b.status[i] = {CPH_ERR_HIP, std::string("first-duplicate read-back: ") + hipGetErrorString(e)};
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess || (b.any_side && hipStreamSynchronize(ctx->side_stream) != hipSuccess))
        return {CPH_ERR_HIP, "hipStreamSynchronize failed"};
    ctx->pool.flush_deferred();
    for (size_t i = 0; i < nj; i++) {
        BuildJob& j = b.jobs[i];
        if (!b.status[i].ok() || j.one_launch()) continue;
        cph_index* ix = j.ix;
        if (j.miss && *(volatile uint32_t*)j.miss) {   // written by the kernels themselves (pinned host memory)
            j.cs_codes.reset();
            j.cs_over = nullptr;
            b.missed.push_back(i);
            continue;
        }
        if (j.cs_over && *(volatile uint32_t*)j.cs_over) { b.overflowed.push_back(i); continue; }
        j.cs_codes.reset();
        ix->first_dup = fd[i] != 0xFFFFFFFFu ? (uint64_t)fd[i] : UINT64_MAX;
        ix->first_dup_dev.reset();
        index_plan_table(ix);
    }
    return {};
}

// The counted window sort of job j overflowed: the same codes again, through narrower windows or the classic passes, into the
// buffers the failed sort left in the index.  Streams: both idle on entry and on exit; the work runs on the ctx's own.
static Status resort_overflowed(cph_ctx* ctx, BuildJob& j) {
    cph_index* ix = j.ix;
    uint32_t* over = j.cs_over;
    j.cs_over = nullptr;
    DevBuf kb = std::move(ix->sorted_codes), va = std::move(ix->perm);
    const Status r = sort_codes_after_overflow(ctx, ix, j.cs_codes, kb, va, over, 2);
    j.cs_codes.reset();
    return r;
}

static void build_run(cph_ctx* ctx, std::vector<BuildJob>& jobs, std::vector<Status>& status);

// A second attempt for job i, alone and on the ctx's own stream: the job leaves the batch, the index forgets the failed attempt,
// the statistics `next` names are launched, a one-job batch runs, the job returns.
// Streams: both idle on entry and on exit.
static void restart_job(Batch& b, size_t i, NextAttempt next) {
    cph_ctx* ctx = b.ctx;
    std::vector<BuildJob> one;
    one.push_back(std::move(b.jobs[i]));
    std::vector<Status> st1(1);
    BuildJob& j = one[0];
    cph_index* ix = j.ix;
    j.side = false;
    j.miss = nullptr;
    j.avoid = next.avoid;
    index_reset_for_rebuild(ix);
    if (next.from == Alphabets::SplitExact) {
        ctx->n_split_respec++;
        st1[0] = codec_try_split(ctx, j.dcols, 1, ix->nrows, nullptr, &ix->codec, false, nullptr);
        if (st1[0].ok() && !ix->codec.has_split()) next.from = Alphabets::ExactStats;   // (the exact statistics want no split after all)
    }
    if (next.from != Alphabets::SplitExact && next.from != Alphabets::ExactStats)
        st1[0] = {CPH_ERR_INVALID, "internal: a restarted build takes exact statistics only"};
    j.from = next.from;
    if (st1[0].ok() && j.from == Alphabets::ExactStats) st1[0] = codec_stats_launch(ctx, j.dcols, j.nkeycols, &j.stats_dev);
    if (st1[0].ok()) build_run(ctx, one, st1);
    b.status[i] = st1[0];
    b.jobs[i] = std::move(one[0]);
}

// Runs a batch of jobs whose phase 1 succeeded (status[i].ok()); status[i] receives each job's outcome.
// Staged input copies are released with the jobs (stream-ordered reuse is safe).
static void build_run(cph_ctx* ctx, std::vector<BuildJob>& jobs, std::vector<Status>& status) {
    Batch b(ctx, jobs, status);
    Status s = enqueue_readbacks(b);
    if (s.ok()) s = sync1_then_phase2(b);
    if (s.ok()) s = sync2_and_read(b);
    if (!s.ok()) {
        for (Status& st : status)
            if (st.ok()) st = s;
        return;
    }
    // both streams are idle from here on; second attempts run one at a time
    for (size_t i : b.overflowed) status[i] = resort_overflowed(ctx, jobs[i]);
    for (size_t i : b.missed) restart_job(b, i, next_attempt(jobs[i]));
    for (size_t i : b.not_small) restart_job(b, i, next_attempt(jobs[i]));   // keys the one-workgroup build could not take
}

Status build_index(cph_ctx* ctx, const cph_strcol* keycols, int32_t nkeycols, cph_index* ix, bool unique) {
    if (nkeycols == 1 && keycols && keycols[0].mem == CPH_MEM_HOST && validate_cols(keycols, nkeycols).ok()) {
        bool taken = false;
        CPH_TRY(build_from_host_codes(ctx, keycols, nkeycols, ix, unique, &taken));   // only the key CODES cross PCIe
        if (taken) return {};
    }
    std::vector<BuildJob> jobs(1);
    std::vector<Status> st(1);
    jobs[0].ix = ix;
    jobs[0].unique = unique;
    st[0] = build_phase1(ctx, keycols, nkeycols, &jobs[0]);
    if (st[0].ok()) build_run(ctx, jobs, st);
    return st[0];
}

void build_indexes(cph_ctx* ctx, const cph_index_spec* specs, int32_t nspecs, cph_index** ixs, Status* st) {
    std::vector<BuildJob> jobs((size_t)nspecs);
    std::vector<Status> status((size_t)nspecs);
    // Two streams for a batch: every second build is enqueued on the side stream, so a small table's launch-latency-bound
    // kernels (products: 1e5 rows, ~15 launches of a few microseconds of work each) run inside the gaps and beside the kernels
    // of its neighbour (customers: 1e7 rows) instead of behind them.  Both streams are idle again when the call returns.
    bool two_streams = nspecs >= 2 && ctx->build_side_stream != 0;
    if (two_streams && !ctx->side_stream && hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        ctx->side_stream = nullptr;
        two_streams = false;
    }
    struct DeferGuard {   // no block changes hands between the two streams' kernels while both run
        cph_ctx* c;
        ~DeferGuard() {
            if (!c) return;
            (void)hipStreamSynchronize(c->stream);
            (void)hipStreamSynchronize(c->side_stream);
            c->pool.end_defer();
        }
    } defer{two_streams ? ctx : nullptr};
    if (two_streams) {
        // The header's promise — all work of a ctx is ordered on the stream set with cph_ctx_set_stream — must hold for the side
        // jobs too: they may read key columns that kernels of the CALLER, queued on ctx->stream, are still producing, and they take
        // pool blocks whose last users run on ctx->stream.  So the side stream first waits for everything enqueued there so far.
        hipError_t fe = ctx->side_fork ? hipSuccess : hipEventCreateWithFlags(&ctx->side_fork, hipEventDisableTiming);
        if (fe == hipSuccess) fe = hipEventRecord(ctx->side_fork, ctx->stream);
        if (fe == hipSuccess) fe = hipStreamWaitEvent(ctx->side_stream, ctx->side_fork, 0);
        if (fe != hipSuccess) {
            (void)hipGetLastError();
            two_streams = false;
            defer.c = nullptr;
        }
    }
    if (two_streams) ctx->pool.begin_defer();
    for (int i = 0; i < nspecs; i++) {
        jobs[(size_t)i].ix = ixs[i] = new (std::nothrow) cph_index();
        jobs[(size_t)i].side = two_streams && (i & 1);
        jobs[(size_t)i].unique = specs[i].unique != 0;
        SideStream on_side(ctx, jobs[(size_t)i].side);
        if (!ixs[i]) status[(size_t)i] = {CPH_ERR_NOMEM, "out of host memory"};
        else status[(size_t)i] = build_phase1(ctx, specs[i].keycols, specs[i].nkeycols, &jobs[(size_t)i]);
    }
    build_run(ctx, jobs, status);
    for (int i = 0; i < nspecs; i++) st[i] = std::move(status[(size_t)i]);
}

}  // namespace cph
