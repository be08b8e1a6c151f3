// kc_api.cpp — the C ABI of include/kc.h except the finish: the context's
// lifecycle and buffers (kc_ctx.h), the count pipeline (FASTQ index -> the
// engines -> records, spill), ingest, output, queries and synth. The finish
// pipeline and the run merging are in kc_finish.cpp.
//
// Replaces PrepareGPU / processKMers / FreeGPU (GPUHandler.cu:397-519) and the
// host aggregation of KMerCounter (KMerCounter.cpp:51-106).
#include <errno.h>
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <sched.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <memory>
#include <new>
#include <thread>

#include "kc_ctx.h"
#include "kc_io.h"

static std::atomic<uint64_t> g_ctx_seq(0);

kc_status fail(kc_ctx* c, kc_status s, const char* fmt, ...) {
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return s;
}

kc_status ensure(kc_ctx* c, DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return KC_OK;
    if (b.p) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        b.release();
    }
    HIPCHK(c, b.alloc(bytes < 256 ? 256 : bytes));
    return KC_OK;
}

// As ensure, but a pooled run buffer that is big enough (best fit) is swapped
// in before anything is allocated: finished runs, merge outputs and fin_packed
// trade the same few large buffers instead of reallocating tens of GB per pass.
kc_status ensure_pooled(kc_ctx* c, DevBuf& b, size_t bytes) {
    if (b.p && b.bytes >= bytes) return KC_OK;
    int best = -1;
    for (size_t i = 0; i < c->run_pool.size(); i++)
        if (c->run_pool[i].bytes >= bytes && (best < 0 || c->run_pool[i].bytes < c->run_pool[(size_t)best].bytes))
            best = (int)i;
    if (best >= 0) {
        DevBuf t = std::move(c->run_pool[(size_t)best]);
        c->run_pool.erase(c->run_pool.begin() + best);
        if (b.p) c->run_pool.push_back(std::move(b));
        b = std::move(t);
        return KC_OK;
    }
    return ensure(c, b, bytes);
}

// fin_packed's buffer leaves for a run (no copy); fin_packed gets a pooled
// buffer back if there is one (grown by the next finish if it is short)
DevBuf take_fin_packed(kc_ctx* c) {
    DevBuf run = std::move(c->fin_packed);
    if (!c->run_pool.empty()) {
        c->fin_packed = std::move(c->run_pool.back());
        c->run_pool.pop_back();
    }
    return run;
}

kc_status sync_stats(kc_ctx* c) {
    HIPCHK(c, hipMemcpyAsync(c->stats_h, c->stats, ST_N * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KC_OK;
}

static uint32_t probe_limit(const kc_ctx* c) {
    // a nearly full table: give up early and spill instead of walking long runs
    uint64_t used = c->stats_h[ST_CLAIMED];
    if (used * 10 >= c->cap * 9) return 8;
    return c->W == 1 ? 128 : 64;
}

// The launch arguments of reads [read0, read0 + nr) of a count call. pre0 >= 0:
// the reads are already encoded in part_codes / part_inval (/ var_rlen) from
// read index pre0 on; else kernel E writes them at the buffers' start.
static CountLaunch make_launch(const kc_ctx* c, const uint8_t* base, const uint64_t* seq_off, uint64_t read0,
                               uint64_t nr, int64_t L, int64_t pre0) {
    CountLaunch l;
    l.base = base;
    l.seq_off = seq_off;
    l.read0 = read0;
    l.n_reads = nr;
    l.L = (int)L;
    l.k = (int)c->k;
    l.table = c->table;
    l.cap = c->cap;
    l.spill = c->spill;
    l.spill_cap = c->spill_cap;
    l.stats = c->stats;
    l.probe_limit = probe_limit(c);
    const uint64_t at = pre0 < 0 ? 0 : (uint64_t)pre0 + read0;
    const uint64_t g0 = at * (uint64_t)groups_per_read((int)L);
    l.codes = c->part_codes.as<uint32_t>() + g0;
    l.inval = c->part_inval.as<uint16_t>() + g0;
    // rows of length 0 (one-pass empty rows) are skipped by P1 / P2
    l.rlen = (pre0 >= 0 && c->var_rlen) ? c->var_rlen + at : nullptr;
    return l;
}

// tpre[r + 1] = tpre[r] + tiles of region r = [rstart[r], rstart[r + 1]), each
// region cut into tiles of its own; returns the tile count
static uint64_t tile_prefix(const uint64_t* rstart, size_t nreg, uint64_t tile, uint64_t* tpre) {
    tpre[0] = 0;
    for (size_t r = 0; r < nreg; r++) tpre[r + 1] = tpre[r] + (rstart[r + 1] - rstart[r] + tile - 1) / tile;
    return tpre[nreg];
}

// ---------------------------------------------------------------------------
// counting
// ---------------------------------------------------------------------------

static kc_status check_line(kc_ctx* c, int64_t L) {
    if (L < c->k) return fail(c, KC_ERR_ARG, "read length %lld is shorter than k=%lld", (long long)L, (long long)c->k);
    if (L > 32767) return fail(c, KC_ERR_ARG, "read length %lld exceeds 32767 (the reference's u16 2L header)",
                               (long long)L);
    return KC_OK;
}

// Engine "table": every k-mer is inserted into the global HBM table with
// atomics. Counts n_reads reads (stride mode when seq_off == nullptr).
static kc_status count_reads_table(kc_ctx* c, const uint8_t* base, const uint64_t* seq_off, uint64_t n_reads,
                                   int64_t L) {
    if (c->count.finished) return fail(c, KC_ERR_STATE, "kc_finish was called; kc_reset first");
    const uint64_t nw = (uint64_t)(L - c->k + 1);
    const uint64_t max_reads = c->spill_cap / nw;
    if (max_reads == 0) return fail(c, KC_ERR_ARG, "gpu_memory_limit too small for one read's windows");
    uint64_t done = 0;
    kc_status s;
    float ms = 0.f;
    Marks mk{c};
    while (done < n_reads) {
        uint64_t free_slots = c->spill_cap - c->stats_h[ST_SPILL_FILL];
        uint64_t nr = n_reads - done;
        if (nr > max_reads) nr = max_reads;
        if (nr * nw > free_slots) {
            if ((s = flush_spill(c))) return s;
        }
        const CountLaunch a = make_launch(c, base, seq_off, done, nr, L, -1);
        HIPCHK(c, mk.begin());
        HIPCHK(c, launch_count_kmers(a, 256 * 16, c->stream));
        HIPCHK(c, mk.mark());
        if ((s = sync_stats(c))) return s;
        HIPCHK(c, mk.add(0, ms));
        c->count.insert_launches++;
        if (c->stats_h[ST_ERR] & ERR_SPILL_OVERFLOW) return fail(c, KC_ERR_INTERNAL, "spill buffer overflow");
        done += nr;
    }
    c->count.insert_ms += ms;
    c->st.last_count_ms = ms;
    c->count.engines_used |= 4u;
    c->st.valid_kmers = c->stats_h[ST_VALID];
    c->st.spilled_kmers = c->count.spilled_flushed + c->stats_h[ST_SPILL_FILL];
    return KC_OK;
}

kc_status grow_records(kc_ctx* c, uint64_t need) {
    if (need <= c->rec_cap) return KC_OK;
    uint64_t ncap = c->rec_cap ? c->rec_cap : 1024;
    while (ncap < need) ncap = ncap + ncap / 2 + 1024;
    const int W = c->W;
    DevArr<uint64_t> nk;
    DevArr<uint32_t> nc;
    DevArr<uint8_t> nd;
    HIPCHK(c, nk.alloc((size_t)W * ncap * 8));
    HIPCHK(c, nc.alloc((size_t)ncap * 4));
    HIPCHK(c, nd.alloc((size_t)ncap + 16));
    if (c->count.rec_n) {
        for (int j = 0; j < W; j++)
            HIPCHK(c, hipMemcpyAsync(nk + (size_t)j * ncap, c->rec_keys + (size_t)j * c->rec_cap, c->count.rec_n * 8,
                                     hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(nc, c->rec_cnts, c->count.rec_n * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(nd, c->rec_dig, c->count.rec_n, hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::swap(c->rec_keys, nk);  // (the old buffers go with nk, nc, nd)
    std::swap(c->rec_cnts, nc);
    std::swap(c->rec_dig, nd);
    c->rec_cap = ncap;
    return KC_OK;
}

// P5 overflowed the record buffer (ERR_REC_OVERFLOW) before anything went to
// the fallback table or the spill, whose inserts are not idempotent: the error
// bit is cleared and the record cursor put back to rec0 (desc0, when given:
// the descriptor fill too), for a rerun with a bigger buffer
static kc_status rerun_reset(kc_ctx* c, uint64_t rec0, const uint64_t* desc0 = nullptr) {
    const uint64_t err = c->stats_h[ST_ERR] & ~(uint64_t)ERR_REC_OVERFLOW;
    HIPCHK(c, hipMemcpyAsync(c->stats + ST_ERR, &err, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->rec_cursor, &rec0, 8, hipMemcpyHostToDevice, c->stream));
    if (desc0) HIPCHK(c, hipMemcpyAsync(c->stats + ST_DESC_FILL, desc0, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (desc0) c->stats_h[ST_DESC_FILL] = *desc0;
    c->stats_h[ST_ERR] = err;
    c->count.rec_n = rec0;
    return KC_OK;
}

static const size_t kMaxLds = 160 * 1024;  // LDS of one CU (gfx950): the P2 workgroup's ceiling
// skm engine cardinality sample: buckets counted first, the smallest batch
// (keys) sampled, and the distinct-key share above which the key-prefix engine
// counts instead
static const uint32_t kSkmSample = 256;
static const uint64_t kSkmSampleMinKeys = 1ull << 24;
static const double kSkmDistinctMax = 0.35;

// The launch wrappers' argument groups, from the context: the record buffer,
// the P5 descriptors, and P5's fallback (the global table, then `spill`, the
// batch's free key buffer of key_cap keys)
RecSink rec_sink(const kc_ctx* c) { return {c->rec_keys, c->rec_cnts, c->rec_cap, c->rec_cursor}; }
DescSink desc_sink(const kc_ctx* c) {
    return {c->desc_key.as<uint64_t>(), c->desc_start.as<uint64_t>(), c->desc_len.as<uint32_t>(), kDescCap};
}
static Fallback p5_fallback(const kc_ctx* c, uint64_t* spill, uint32_t probe_limit) {
    return {c->table, c->cap, spill, c->key_cap, c->stats, probe_limit};
}

// P5s direct (high cardinality, empty record state): sort_runs_k writes the
// batch's records straight into fin_packed as a finished sorted run (record
// 0: key 0 when present), each run of sub-buckets at its first key's position;
// runs that held equal keys leave gaps that a segment copy closes. With
// key-range passes (count_reads_part) every pass appends its key range at
// record pk_at (the records of the earlier passes); `last` keeps fin_packed as
// the finished run (direct_keep) and the record state stays empty. *done =
// false when runs were handed to the hash path: nothing of this batch was
// kept and the caller counts it into records as usual. `total` sizes
// fin_packed on the first pass (keys of all passes).
static kc_status direct_keep(kc_ctx* c, uint64_t nrec);
static kc_status p5s_direct(kc_ctx* c, const uint64_t* keys, uint64_t kstride, const uint64_t* sub_starts, uint32_t nb,
                            uint64_t n,
                            uint8_t* rf, size_t fl, bool* done, uint64_t* records, float* ms, uint64_t pk_at = 0,
                            uint64_t total = 0, bool last = true) {
    kc_status s;
    *done = false;
    const int W = c->W;
    const size_t rs = (size_t)c->rs;
    uint8_t* bf = rf + ((size_t)nb << 8);
    uint32_t* nflag = (uint32_t*)(bf + nb);
    // (inside a flush of padded / one-pass rows: key 0's presence from the reads)
    if ((s = c->var_rlen ? recompute_presence(c) : sync_stats(c))) return s;
    const bool key0 = c->stats_h[ST_KEY0_PRESENT] != 0;
    const uint64_t off0 = key0 ? 1 : 0;
    if (pk_at == 0 && (s = ensure_pooled(c, c->fin_packed, (off0 + (total > n ? total : n)) * rs + 16))) return s;
    if (c->fin_packed.bytes < (off0 + pk_at + n) * rs) return fail(c, KC_ERR_INTERNAL, "key-range pass overflows its run");
    HIPCHK(c, hipMemsetAsync(rf, 0, fl, c->stream));
    Marks mk{c};
    HIPCHK(c, mk.begin());
    HIPCHK(c, launch_sort_runs(W, keys, kstride, sub_starts, nb, rec_sink(c), c->stats, desc_sink(c), rf, bf, nflag,
                               2 * c->n_cu, c->stream, c->fin_packed.p, off0 + pk_at));
    HIPCHK(c, mk.mark());
    uint32_t nf = 0;
    uint64_t R = 0;
    HIPCHK(c, hipMemcpyAsync(&nf, nflag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&R, c->rec_cursor, 8, hipMemcpyDeviceToHost, c->stream));
    if ((s = sync_stats(c))) return s;
    HIPCHK(c, mk.ms(0, ms));
    *records = R;
    const uint64_t ndesc = c->stats_h[ST_DESC_FILL];
    auto clear_cursor = [&]() -> kc_status {
        // record cursor and descriptors start empty again
        HIPCHK(c, hipMemsetAsync(c->rec_cursor, 0, 8, c->stream));
        c->stats_h[ST_DESC_FILL] = 0;
        HIPCHK(c, hipMemcpyAsync(c->stats + ST_DESC_FILL, &c->stats_h[ST_DESC_FILL], 8, hipMemcpyHostToDevice,
                                 c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return KC_OK;
    };
    if (nf || (R < n && ndesc > kDescCap)) return clear_cursor();  // undo: the caller counts into records
    if (R < n) {
        // equal keys in some runs: close the gaps (segments in key order) into
        // merge_tmp, then back to the pass's place
        if ((s = ensure(c, c->desc_k2, ndesc * 8)) || (s = ensure(c, c->desc_v, ndesc * 4)) ||
            (s = ensure(c, c->desc_v2, ndesc * 4)) || (s = ensure(c, c->desc_lens, ndesc * 8)) ||
            (s = ensure(c, c->desc_offs, ndesc * 8)) || (s = ensure(c, c->rle_tmp, scan_tmp_elems(ndesc) * 8)) ||
            (s = ensure_pooled(c, c->merge_tmp, R * rs + 16)))
            return s;
        HIPCHK(c, launch_iota_u32(c->desc_v.as<uint32_t>(), ndesc, c->stream));
        int which = 0;
        if ((s = sort_records(c, c->desc_key.as<uint64_t>(), c->desc_k2.as<uint64_t>(), c->desc_v.as<uint32_t>(),
                              c->desc_v2.as<uint32_t>(), ndesc, ndesc, &which, 1)))
            return s;
        const uint32_t* order = (which ? c->desc_v2 : c->desc_v).as<uint32_t>();
        HIPCHK(c, launch_desc_prep(order, c->desc_len.as<uint32_t>(), ndesc, c->desc_lens.as<uint64_t>(),
                                   c->stream));
        HIPCHK(c, launch_scan_u64(c->desc_lens.as<uint64_t>(), c->desc_offs.as<uint64_t>(), ndesc,
                                  c->rle_tmp.as<uint64_t>(), c->stream));
        HIPCHK(c, launch_packed_seg_copy(W, c->fin_packed.p, c->merge_tmp.p, order, c->desc_start.as<uint64_t>(),
                                         c->desc_len.as<uint32_t>(), c->desc_offs.as<uint64_t>(), ndesc, 0,
                                         4 * c->n_cu, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->fin_packed.as<uint8_t>() + (off0 + pk_at) * rs, c->merge_tmp.p, R * rs,
                                 hipMemcpyDeviceToDevice, c->stream));
    }
    if ((s = clear_cursor())) return s;
    *done = true;
    return last ? direct_keep(c, pk_at + R) : KC_OK;
}

// fin_packed, written by direct passes (nrec records after the key-0 slot),
// becomes a finished sorted run
static kc_status direct_keep(kc_ctx* c, uint64_t nrec) {
    kc_status s;
    if ((s = c->var_rlen ? recompute_presence(c) : sync_stats(c))) return s;
    const bool key0 = c->stats_h[ST_KEY0_PRESENT] != 0;
    std::vector<uint32_t> r0((size_t)c->rs / 4, 0u);
    if (key0) {
        r0.back() = (uint32_t)c->stats_h[ST_KEY0];
        HIPCHK(c, hipMemcpyAsync(c->fin_packed.p, r0.data(), c->rs, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->count.batches = 1;  // this batch: moved to batches_cut with the run
    return keep_finished_run(c, (key0 ? 1 : 0) + nrec);
}

// Key-range passes (high cardinality): when one batch cannot hold the keys of
// all reads, the reads are not cut into batches whose sorted runs must then be
// merged; the key space is cut instead. A P1 pass over all reads counts the
// live keys by their top byte (word0 >> 56); consecutive top bytes are
// grouped into passes of at most key_cap keys, balanced; each pass re-walks all
// reads and keeps only its key range (P1/P2 filter), and P5s direct writes it
// after the previous passes' records: the runs are disjoint key ranges in key
// order, so the finished run is their concatenation (no merge). Returns the
// pass bounds (empty: not applicable, count by read batches).
static kc_status plan_key_passes(kc_ctx* c, CountLaunch l, int64_t L, std::vector<uint32_t>* kp, uint64_t* keys) {
    kp->clear();
    kc_status s;
    PartGeom pg = part_geometry((int)L, (int)c->k, l.n_reads);
    const uint64_t hn = 256 * pg.nseg;
    constexpr uint32_t NG = 16;  // key groups: word0 >> 60
    if ((s = ensure(c, c->part_ghist, (NG * hn + NG) * 8))) return s;
    uint64_t* gh = c->part_ghist.as<uint64_t>();
    Marks mk{c};
    HIPCHK(c, mk.begin());
    HIPCHK(c, launch_part_hist(l, pg, gh, 48, c->stream, 4));
    HIPCHK(c, launch_hist_group_totals(gh, pg.nseg, NG, gh + NG * hn, c->stream));
    std::vector<uint64_t> gt(NG);
    HIPCHK(c, hipMemcpyAsync(gt.data(), gh + NG * hn, NG * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, mk.mark());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, mk.add(0, c->count.part_ms[0]));
    uint64_t total = 0;
    for (uint64_t x : gt) total += x;
    *keys = total;
    if (total <= c->key_cap) return KC_OK;
    uint64_t np = (total + c->key_cap - 1) / c->key_cap;
    // (KC_KEY_PASSES_MIN: path selector for tests and measurements, same counts)
    if (const char* e = test_hook("KC_KEY_PASSES_MIN")) np = std::max<uint64_t>(np, strtoull(e, nullptr, 10));
    const uint64_t cap = std::min<uint64_t>(c->key_cap, (total + np - 1) / np * 5 / 4);
    const uint64_t target = (total + np - 1) / np;
    std::vector<uint32_t> bounds{0};
    uint64_t acc = 0;
    for (uint32_t g = 0; g < NG; g++) {
        const uint64_t x = gt[g];
        if (x > c->key_cap) return KC_OK;  // one group holds more than a batch: read batches
        // (a group above the balanced cap but within a batch gets a pass of its own)
        // close the pass before g when g would overflow it, or when stopping
        // here is closer to the balanced target than taking g
        if (acc > 0 && (acc + x > cap || (acc + x > target && acc + x - target > target - acc))) {
            bounds.push_back(g * (256 / NG));
            acc = 0;
        }
        acc += x;
    }
    bounds.push_back(256);
    if (bounds.size() - 1 > 16) return KC_OK;
    *kp = bounds;
    return KC_OK;
}

// Smallest batch (keys) that takes the P3b pre-split (high cardinality);
// KC_P3B_MIN: path selector for tests, same counts either way
static uint64_t p3b_min_of() {
    uint64_t m = 1ull << 22;
    if (const char* e = test_hook("KC_P3B_MIN")) m = strtoull(e, nullptr, 10);
    return m;
}

// Engine "partition": per batch of reads
//   P1 hist   : digit (word0 >> 48) & 255 per segment of reads
//   P2 scatter: keys to their digit's region (LDS counting sort per tile)
//   P3        : regional scatter on digit (word0 >> 56) -> grouped by bucket =
//               word0 >> 48, the key's first 8 bases: buckets are in key order
//   P4        : bucket ranges (binary search)
//   P5        : per-bucket LDS hash count -> (key, count) records
// pre0 >= 0: the reads are already encoded (fq_encode) in part_codes /
// part_inval from read index pre0 on; kernel E is skipped
//
// The driver (count_reads_part) is the batch loop; the stages below pass
// their results on in a PartBatch.

// Key-range passes of one call (plan_key_passes): high cardinality, all reads
// encoded, more keys than one batch holds, and an empty record state (P5s direct)
struct KeyPasses {
    std::vector<uint32_t> kp;  // pass bounds on word0 >> 56 (empty: the call counts by read batches)
    size_t kpi = 0;            // current pass
    uint64_t keys = 0;         // live keys of all passes
    uint64_t out = 0;          // records the direct passes wrote so far
    bool direct = false;       // every pass so far went direct
    // two passes per walk: P2 writes the second pass's keys (SoA, stride = its
    // key count, then its digit bytes) into fin_packed past the records the
    // first pass will write; that pass's P3 reads them from there
    size_t u_pass = ~(size_t)0;  // the pass whose P2 output is at u_keys
    uint64_t* u_keys = nullptr;
    uint64_t u_n = 0;
    bool on() const { return !kp.empty(); }
    bool last() const { return kpi + 2 == kp.size(); }
};

// One batch of reads (or one key-range pass over all of them)
struct PartBatch {
    CountLaunch l;
    PartGeom pg;
    // KC_P2_NO_DIGS (measurement): P2 writes no digit bytes (P3 reads word 0)
    bool p2_no_digs = false;
    // P2 writes each key as W consecutive words (one stream per digit run
    // instead of W); P3's scatter reads them so (KC_P2_SOA: the SoA layout,
    // for comparison)
    bool p2_aos = false;
    // P2's output: keys_a (+ digs), or fin_packed when the previous pass's
    // walk wrote it (from_u: two passes per walk)
    bool from_u = false;
    uint64_t* p2_keys = nullptr;
    uint64_t p2_stride = 0;
    const uint8_t* p2_digs = nullptr;
    const uint64_t* p2_base = nullptr;  // P2's run starts (the scanned P1 histogram)
    uint64_t n = 0;                     // keys
    bool p3b = false;             // a P3b pass follows P3 (decided once: P3's output layout and P5's input depend on it)
    uint8_t* p3b_digs = nullptr;  // P3b digit bytes written by P3 (else P3b reads word 0)
    bool p3_aos = false;          // P3's output keys AoS (only when P3b follows)
    // P5's input: P3's output, or P3b's (then with the sub-bucket starts)
    uint64_t* p5_keys = nullptr;
    uint64_t p5_stride = 0;  // 0: AoS (P3's or P3b's output)
    uint64_t* p5_spill = nullptr;
    const uint64_t* sub_starts = nullptr;
};

// E + P1 + P2 of the batch: b.n keys at b.p2_keys. A key-range pass whose keys
// the previous pass's walk wrote (two passes per walk) launches nothing.
static kc_status part_p1_p2(kc_ctx* c, int64_t pre0, KeyPasses& kp, PartBatch& b) {
    kc_status s;
    const int W = c->W;
    CountLaunch& l = b.l;
    const PartGeom& pg = b.pg;
    const bool kpass = kp.on();
    const size_t kpi = kp.kpi;
    Marks mk{c};
    const uint64_t hn = 256 * pg.nseg;
    if ((s = ensure(c, c->part_hist, hn * 8)) || (s = ensure(c, c->part_base, hn * 8)) ||
        (s = ensure(c, c->part_tmp, scan_tmp_elems(hn) * 8)))
        return s;
    const uint64_t ng = l.n_reads * (uint64_t)groups_per_read(l.L);
    if (pre0 < 0 && ((s = ensure(c, c->part_codes, ng * 4 + 16)) || (s = ensure(c, c->part_inval, ng * 2 + 16))))
        return s;
    if (pre0 < 0) {  // (buffers may have moved)
        l.codes = c->part_codes.as<uint32_t>();
        l.inval = c->part_inval.as<uint16_t>();
    }
    b.from_u = kpass && kp.u_pass == kpi;
    b.p2_keys = b.from_u ? kp.u_keys : c->keys_a;
    b.p2_stride = b.from_u ? kp.u_n : c->key_cap;
    b.p2_digs = b.from_u ? (const uint8_t*)(kp.u_keys + (size_t)W * kp.u_n) : c->digs;
    b.p2_base = (b.from_u ? c->part_base2 : c->part_base).as<uint64_t>();
    b.n = b.from_u ? kp.u_n : 0;
    if (b.from_u) return KC_OK;
    const bool dual = kpass && kp.direct && kpi + 2 < kp.kp.size() && !test_hook("KC_NO_DUAL_PASS");
    if (dual && (s = ensure(c, c->part_base2, hn * 8))) return s;
    uint64_t* hist = c->part_hist.as<uint64_t>();
    HIPCHK(c, mk.begin());
    if (pre0 < 0)
        HIPCHK(c, launch_encode_reads(l, c->part_codes.as<uint32_t>(), c->part_inval.as<uint16_t>(), c->stream));
    if (kpass)  // the pass's histogram from the planner's grouped one (no walk)
        HIPCHK(c, launch_hist_group_sum(c->part_ghist.as<uint64_t>(), pg.nseg, l.flo / 16, l.fhi / 16, hist,
                                        c->stream));
    else
        HIPCHK(c, launch_part_hist(l, pg, hist, 48, c->stream));
    HIPCHK(c, launch_scan_u64(hist, c->part_base.as<uint64_t>(), hn, c->part_tmp.as<uint64_t>(), c->stream));
    uint64_t tail[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(&tail[0], c->part_base.as<uint64_t>() + hn - 1, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&tail[1], hist + hn - 1, 8, hipMemcpyDeviceToHost, c->stream));
    if (dual) {
        HIPCHK(c, launch_hist_group_sum(c->part_ghist.as<uint64_t>(), pg.nseg, kp.kp[kpi + 1] / 16,
                                        kp.kp[kpi + 2] / 16, hist, c->stream));
        HIPCHK(c, launch_scan_u64(hist, c->part_base2.as<uint64_t>(), hn, c->part_tmp.as<uint64_t>(), c->stream));
        HIPCHK(c, hipMemcpyAsync(&tail[2], c->part_base2.as<uint64_t>() + hn - 1, 8, hipMemcpyDeviceToHost,
                                 c->stream));
        HIPCHK(c, hipMemcpyAsync(&tail[3], hist + hn - 1, 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, mk.mark());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, mk.add(0, c->count.part_ms[0]));
    const uint64_t n = tail[0] + tail[1];
    if (n > c->key_cap) return fail(c, KC_ERR_INTERNAL, "batch keys %llu exceed capacity", (unsigned long long)n);
    b.n = n;
    // the second pass's keys go past the records this pass will write
    // (key 0 slot + the earlier passes' records + this pass's keys)
    uint64_t* u = nullptr;
    const uint64_t n2 = tail[2] + tail[3];
    if (dual) {
        const size_t at = ((1 + kp.out + n) * (size_t)c->rs + 15) & ~(size_t)15;
        if (at + n2 * (8 * (size_t)W + 1) <= c->fin_packed.bytes && n2 > 0)
            u = (uint64_t*)(c->fin_packed.as<uint8_t>() + at);
    }
    if (u) {
        l.fhi = kp.kp[kpi + 2];  // the walk keeps both passes' ranges
    }
    HIPCHK(c, mk.begin());
    // (p2_no_digs: P2 writes no digit bytes, P3's histogram reads word 0)
    HIPCHK(c, launch_part_scatter(l, pg, c->part_base.as<uint64_t>(), c->keys_a, c->key_cap, 48,
                                  b.p2_no_digs ? nullptr : c->digs.as<uint8_t>(), c->stream,
                                  u ? c->part_base2.as<uint64_t>() : nullptr, u, u ? n2 : 0,
                                  u && !b.p2_no_digs ? (uint8_t*)(u + (size_t)W * n2) : nullptr,
                                  u ? kp.kp[kpi + 1] : 256u, b.p2_aos));
    HIPCHK(c, mk.mark());
    HIPCHK(c, hipEventSynchronize(mk.last()));
    HIPCHK(c, mk.add(0, c->count.part_ms[1], c->count.insert_ms));
    c->count.insert_launches++;
    if (u) {
        kp.u_pass = kpi + 1;
        kp.u_keys = u;
        kp.u_n = n2;
    }
    return KC_OK;
}

// P3 + P4: the keys grouped by bucket in keys_b, the bucket bounds in part_starts
static kc_status part_p3(kc_ctx* c, PartBatch& b) {
    kc_status s;
    const int W = c->W;
    const uint64_t n = b.n;
    Marks mk{c};
    // P3 tiles: regions (P2 digits) cut into tiles of their own
    std::vector<uint64_t> rt(2 * 257);
    HIPCHK(c, hipMemcpy2DAsync(rt.data(), 8, b.p2_base, b.pg.nseg * 8, 8, 256, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rt[256] = n;
    const uint64_t tile = (uint64_t)rp_tile(W, false);
    const uint64_t ntiles = tile_prefix(rt.data(), 256, tile, rt.data() + 257);
    if ((s = ensure(c, c->part_sort_hist, (256 * ntiles + rp_tmp_elems(ntiles) + 2 * 257) * 8))) return s;
    uint64_t* p3h = c->part_sort_hist.as<uint64_t>();
    uint64_t* p3t = p3h + 256 * ntiles + rp_tmp_elems(ntiles);
    HIPCHK(c, hipMemcpyAsync(p3t, rt.data(), 2 * 257 * 8, hipMemcpyHostToDevice, c->stream));
    const RegionTable reg = {p3t, p3t + 257, 256, ntiles, (uint32_t)tile};
    HIPCHK(c, mk.begin());
    // tile histograms from P2's digit bytes (p2_no_digs: from word 0, bits 56..63)
    HIPCHK(c, launch_rp_hist(b.p2_no_digs ? nullptr : b.p2_digs, b.p2_keys, 56, reg, p3h, p3h + 256 * ntiles,
                             2 * c->n_cu, c->stream));
    HIPCHK(c, mk.mark());
    HIPCHK(c, hipEventSynchronize(mk.last()));
    HIPCHK(c, mk.add(0, c->count.part_ms[3]));
    HIPCHK(c, mk.begin());
    b.p3b = c->count.hc_hint && n >= p3b_min_of() && !test_hook("KC_NO_P3B");
    // P3's scatter is the radix scatter by word0 >> 56 over the 256 P2
    // regions. When a P3b pass follows (high cardinality), P3 writes each
    // key's P3b digit byte (bits 40..47) into the free P2 digit array, so
    // P3b's histogram reads 1 B per key, not word 0
    b.p3b_digs = b.p3b ? c->digs.as<uint8_t>() : nullptr;
    // ... and writes the keys AoS for it (P3b reads them so)
    b.p3_aos = b.p3b_digs && !test_hook("KC_P3_SOA");
    HIPCHK(c, launch_rp_scatter(W, false, b.p2_keys, b.p2_aos ? 0 : b.p2_stride, c->keys_b,
                                b.p3_aos ? 0 : c->key_cap, nullptr, nullptr, reg, p3h, 56, b.p3b_digs, 40,
                                2 * c->n_cu, c->stream));
    HIPCHK(c, mk.mark());
    HIPCHK(c, hipEventSynchronize(mk.last()));
    HIPCHK(c, mk.add(0, c->count.part_ms[2]));
    c->count.part_keys += n;

    const uint32_t nb = 1u << kBucketBits;
    if ((s = ensure(c, c->part_starts, ((size_t)nb + 1) * 8))) return s;
    HIPCHK(c, mk.begin());
    HIPCHK(c, launch_bucket_bounds(W, c->keys_b, b.p3_aos ? 0 : c->key_cap, n, kBucketBits,
                                   c->part_starts.as<uint64_t>(), c->stream));
    HIPCHK(c, mk.mark());
    HIPCHK(c, hipEventSynchronize(mk.last()));
    HIPCHK(c, mk.add(0, c->count.part_ms[3]));
    b.p5_keys = c->keys_b;
    b.p5_stride = b.p3_aos ? 0 : c->key_cap;
    b.p5_spill = c->keys_a;
    b.sub_starts = nullptr;
    return KC_OK;
}

// P3b (high cardinality: most keys distinct): every bucket split once more by
// key bits 40..47 (a regional radix pass keys_b -> keys_a over the 65536
// buckets), so P5 counts runs of consecutive sub-buckets in one pass each and
// reads every key once instead of once per sub-range pass
static kc_status part_p3b(kc_ctx* c, PartBatch& b) {
    kc_status s;
    const int W = c->W;
    const uint32_t nb = 1u << kBucketBits;
    Marks mk{c};
    // P3's AoS output always comes with its digit bytes (the
    // regional histogram reads word 0 from SoA keys only)
    if (b.p3_aos && !b.p3b_digs) return fail(c, KC_ERR_INTERNAL, "P3b: AoS keys without digit bytes");
    // the bucket bounds, then each bucket's tile prefix
    std::vector<uint64_t> rt(2 * ((size_t)nb + 1));
    HIPCHK(c, hipMemcpyAsync(rt.data(), c->part_starts.p, ((size_t)nb + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t tile = (uint64_t)rp_tile(W, false);
    const uint64_t nt = tile_prefix(rt.data(), nb, tile, rt.data() + nb + 1);
    const size_t pos_n = 256 * nt, cnt_n = (256 * nt + 1) / 2;
    if ((s = ensure(c, c->p3b_buf, (pos_n + cnt_n + rt.size()) * 8)) ||
        (s = ensure(c, c->sub_starts, (((size_t)nb << 8) + 1) * 8)))
        return s;
    uint64_t* pos = c->p3b_buf.as<uint64_t>();
    uint32_t* cnt_t = (uint32_t*)(pos + pos_n);
    uint64_t* rtd = pos + pos_n + cnt_n;
    HIPCHK(c, hipMemcpyAsync(rtd, rt.data(), rt.size() * 8, hipMemcpyHostToDevice, c->stream));
    const RegionTable reg = {rtd, rtd + nb + 1, (int)nb, nt, (uint32_t)tile};
    HIPCHK(c, mk.begin());
    HIPCHK(c, launch_rp_hist_regional(c->keys_b, 40, reg, pos, cnt_t, 2 * c->n_cu, c->stream, b.p3b_digs));
    // (its output AoS too, for P5s / the hash path; KC_P3B_SOA: arrays)
    const bool p3b_aos = !test_hook("KC_P3B_SOA");
    HIPCHK(c, launch_rp_scatter(W, false, c->keys_b, b.p3_aos ? 0 : c->key_cap, c->keys_a, p3b_aos ? 0 : c->key_cap,
                                nullptr, nullptr, reg, pos, 40, nullptr, 0, 2 * c->n_cu, c->stream));
    HIPCHK(c, launch_sub_starts(rtd, rtd + nb + 1, pos, nb, b.n, c->sub_starts.as<uint64_t>(), c->stream));
    HIPCHK(c, mk.mark());
    HIPCHK(c, hipEventSynchronize(mk.last()));
    HIPCHK(c, mk.add(0, c->count.part_ms[2], c->count.presplit_ms));
    c->count.presplit_batches++;
    b.p5_keys = c->keys_a;
    b.p5_stride = p3b_aos ? 0 : c->key_cap;
    b.p5_spill = c->keys_b;
    b.sub_starts = c->sub_starts.as<uint64_t>();
    return KC_OK;
}

// P5s direct (p5s_direct) on the batch's pre-split keys. kp: the call's
// key-range passes, whose current pass is appended to the direct run of the
// earlier ones. *kept = false: nothing was kept, the batch counts into records.
static kc_status part_p5_direct(kc_ctx* c, const PartBatch& b, const KeyPasses* kp, bool* kept, uint64_t* R) {
    kc_status s;
    const uint32_t nb = 1u << kBucketBits;
    const size_t fl = ((size_t)nb << 8) + nb + 16;
    if ((s = ensure(c, c->run_flags, fl))) return s;
    float t5 = 0.f;
    if ((s = p5s_direct(c, b.p5_keys, b.p5_stride, b.sub_starts, nb, b.n, c->run_flags.as<uint8_t>(), fl, kept, R, &t5,
                        kp ? kp->out : 0, kp ? kp->keys : 0, kp ? kp->last() : true)))
        return s;
    c->count.part_ms[4] += t5;
    c->count.p5_launches++;
    if (debug_on() && kp)
        fprintf(stderr, "kc: P5s direct pass %zu [%u, %u) n=%llu records=%llu kept=%d %.3f ms\n", kp->kpi,
                kp->kp[kp->kpi], kp->kp[kp->kpi + 1], (unsigned long long)b.n, (unsigned long long)*R, *kept ? 1 : 0,
                t5);
    else if (debug_on())
        fprintf(stderr, "kc: P5s direct n=%llu records=%llu kept=%d %.3f ms\n", (unsigned long long)b.n,
                (unsigned long long)*R, *kept ? 1 : 0, t5);
    return KC_OK;
}

// P5s into records: pre-split runs sorted in LDS (records <= keys, no
// overflow); the runs it flags (a sub-bucket too big, clustered keys) take the
// LDS hash table
static kc_status part_p5_sorted(kc_ctx* c, const PartBatch& b, uint64_t rec0) {
    kc_status s;
    const int W = c->W;
    const uint32_t nb = 1u << kBucketBits;
    float t = 0.f;
    Marks mk{c};
    if ((s = grow_records(c, rec0 + b.n))) return s;
    const size_t fl = ((size_t)nb << 8) + nb + 16;
    if ((s = ensure(c, c->run_flags, fl))) return s;
    uint8_t* rf = c->run_flags.as<uint8_t>();
    uint8_t* bf = rf + ((size_t)nb << 8);
    uint32_t* nflag = (uint32_t*)(bf + nb);
    HIPCHK(c, hipMemsetAsync(rf, 0, fl, c->stream));
    HIPCHK(c, mk.begin());
    HIPCHK(c, launch_sort_runs(W, b.p5_keys, b.p5_stride, b.sub_starts, nb, rec_sink(c), c->stats, desc_sink(c), rf,
                               bf, nflag, 2 * c->n_cu, c->stream));
    uint32_t nf = 0;
    HIPCHK(c, hipMemcpyAsync(&nf, nflag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nf)
        HIPCHK(c, launch_count_buckets(W, b.p5_keys, b.p5_stride, c->part_starts.as<uint64_t>(), nb, rec_sink(c),
                                       p5_fallback(c, b.p5_spill, b.l.probe_limit), c->cfg.lds_slots, c->n_cu,
                                       desc_sink(c), c->stream, true, b.sub_starts, rf, bf,
                                       (uint32_t)sort_runs_keys(W)));
    HIPCHK(c, mk.mark());
    HIPCHK(c, hipMemcpyAsync(&c->count.rec_n, c->rec_cursor, 8, hipMemcpyDeviceToHost, c->stream));
    if ((s = sync_stats(c))) return s;
    HIPCHK(c, mk.ms(0, &t));
    c->count.part_ms[4] += t;
    c->count.p5_launches++;
    c->count.sorted_run_batches++;
    if (debug_on())
        fprintf(stderr, "kc: P5s n=%llu runs=%llu flagged=%u records=%llu %.3f ms\n", (unsigned long long)b.n,
                (unsigned long long)c->stats_h[ST_P5_PASSES], nf, (unsigned long long)c->count.rec_n, t);
    if (c->stats_h[ST_ERR] & ERR_REC_OVERFLOW) return fail(c, KC_ERR_INTERNAL, "record buffer overflow");
    return KC_OK;
}

// P5 by LDS hash table. Records: at most one LDS table per bucket unless
// buckets were split into sub-range passes (high cardinality); on overflow P5
// reruns with a bigger buffer (safe while nothing went to the fallback table
// or the spill, whose inserts are not idempotent).
static kc_status part_p5_hash(kc_ctx* c, const PartBatch& b, uint64_t rec0) {
    kc_status s;
    const int W = c->W;
    const uint32_t nb = 1u << kBucketBits;
    const uint64_t n = b.n;
    float t = 0.f;
    Marks mk{c};
    uint64_t bound = (uint64_t)nb * (uint64_t)bucket_lds_slots(W);
    if (bound > n || c->count.hc_hint) bound = n;  // high cardinality: about one record per key
    const uint64_t claimed0 = c->stats_h[ST_CLAIMED];
    const uint64_t desc0 = c->stats_h[ST_DESC_FILL];
    for (;;) {
        if ((s = grow_records(c, rec0 + bound))) return s;
        // keys_a is free after P3: it takes P5's spills (capacity >= n)
        HIPCHK(c, mk.begin());
        HIPCHK(c, launch_count_buckets(W, b.p5_keys, b.p5_stride, c->part_starts.as<uint64_t>(), nb, rec_sink(c),
                                       p5_fallback(c, b.p5_spill, b.l.probe_limit), c->cfg.lds_slots, c->n_cu,
                                       desc_sink(c), c->stream, c->count.hc_hint, b.sub_starts));
        HIPCHK(c, mk.mark());
        HIPCHK(c, hipMemcpyAsync(&c->count.rec_n, c->rec_cursor, 8, hipMemcpyDeviceToHost, c->stream));
        if ((s = sync_stats(c))) return s;
        HIPCHK(c, mk.ms(0, &t));
        c->count.part_ms[4] += t;
        c->count.p5_launches++;
        if (debug_on())
            fprintf(stderr, "kc: P5 n=%llu passes=%llu aborts=%llu max_m=%llu records=%llu %.3f ms\n",
                    (unsigned long long)n, (unsigned long long)c->stats_h[ST_P5_PASSES],
                    (unsigned long long)c->stats_h[ST_P5_ABORTS], (unsigned long long)c->stats_h[ST_P5_MAXM],
                    (unsigned long long)c->count.rec_n, t);
        if (!(c->stats_h[ST_ERR] & ERR_REC_OVERFLOW)) return KC_OK;
        if (bound >= n || c->stats_h[ST_CLAIMED] != claimed0 || c->stats_h[ST_SPILL2_FILL])
            return fail(c, KC_ERR_INTERNAL, "record buffer overflow");
        bound = n;
        if ((s = rerun_reset(c, rec0, &desc0))) return s;
    }
}

// The partition engine's driver: the batch (or key-range pass) loop over the
// stages above, the choice of P5's form, and the batch bookkeeping
static kc_status count_reads_part(kc_ctx* c, const uint8_t* base, const uint64_t* seq_off, uint64_t n_reads,
                                  int64_t L, int64_t pre0) {
    if (c->count.finished) return fail(c, KC_ERR_STATE, "kc_finish was called; kc_reset first");
    const uint64_t nw = (uint64_t)(L - c->k + 1);
    const uint64_t max_reads = c->key_cap / nw;
    if (max_reads == 0) return fail(c, KC_ERR_ARG, "gpu_memory_limit too small for one read's windows");
    kc_status s;
    uint64_t done = 0;
    KeyPasses kp;
    const bool p2_no_digs = test_hook("KC_P2_NO_DIGS") != nullptr;
    const bool p2_aos = !p2_no_digs && !test_hook("KC_P2_SOA");
    if (pre0 >= 0 && c->count.hc_hint && nw * n_reads > c->key_cap && c->count.rec_n == 0 && c->count.batches == 0 &&
        c->stats_h[ST_CLAIMED] == 0 && !c->count.skm_used && c->runs.empty() && !test_hook("KC_NO_KEY_PASSES") &&
        !test_hook("KC_NO_P3B") && !test_hook("KC_NO_SORT_RUNS") && !test_hook("KC_NO_P5S_DIRECT")) {
        if ((s = plan_key_passes(c, make_launch(c, base, seq_off, 0, n_reads, L, pre0), L, &kp.kp, &kp.keys)))
            return s;
        kp.direct = kp.on();
        if (kp.on()) c->count.key_passes += kp.kp.size() - 1;
        // the finished run's buffer (key 0 slot + every key), before the first
        // walk: it holds the second pass's P2 output until that pass's P3
        if (kp.on() && (s = ensure_pooled(c, c->fin_packed, (1 + kp.keys) * (size_t)c->rs + 16))) return s;
        if (debug_on() && kp.on())
            fprintf(stderr, "kc: %zu key-range passes over %llu keys\n", kp.kp.size() - 1,
                    (unsigned long long)kp.keys);
    }
    uint64_t direct_min = 1ull << 22;  // (KC_P5S_DIRECT_MIN: path selector for tests)
    if (const char* e = test_hook("KC_P5S_DIRECT_MIN")) direct_min = strtoull(e, nullptr, 10);
    while (done < n_reads) {
        const bool kpass = kp.on();
        uint64_t nr = n_reads - done;
        if (nr > max_reads && !kpass) nr = max_reads;
        PartBatch b;
        b.l = make_launch(c, base, seq_off, done, nr, L, pre0);
        if (kpass) {
            b.l.flo = kp.kp[kp.kpi];
            b.l.fhi = kp.kp[kp.kpi + 1];
            b.l.no_stats = kp.kpi > 0;
        }
        b.pg = part_geometry((int)L, (int)c->k, nr);
        b.p2_no_digs = p2_no_digs;
        b.p2_aos = p2_aos;
        if ((s = part_p1_p2(c, pre0, kp, b))) return s;
        if (experiment_knob("KC_P2_SKIP")) {  // keys are invalid, stop after P2
            c->count.batches++;
            done += nr;
            continue;
        }
        if (b.n > 0) {
            if ((s = part_p3(c, b)) || (b.p3b && (s = part_p3b(c, b)))) return s;
            const uint64_t rec0 = c->count.rec_n;
            if ((s = ensure(c, c->desc_key, kDescCap * 8)) || (s = ensure(c, c->desc_start, kDescCap * 8)) ||
                (s = ensure(c, c->desc_len, kDescCap * 4)))
                return s;
            // (KC_NO_SORT_RUNS: hash table for all runs)
            const bool sort_runs = b.sub_starts && !test_hook("KC_NO_SORT_RUNS");
            bool dd = false;  // P5s direct kept the batch: no records
            uint64_t R = 0;
            if (kpass && kp.direct) {
                // key-range pass: appended to the direct run of the earlier passes
                if (sort_runs && (s = part_p5_direct(c, b, &kp, &dd, &R))) return s;
                if (dd) {
                    kp.out += R;
                    c->count.engines_used |= 2u;
                    if (!kp.last()) {
                        kp.kpi++;
                        continue;
                    }
                    c->count.sorted_run_batches++;
                    done += nr;
                    continue;
                }
                // this pass cannot go direct: the earlier passes become a
                // finished run, this pass and the later ones count into records
                kp.direct = false;
                if (kp.out > 0 && (s = direct_keep(c, kp.out))) return s;
            }
            if (!kpass && sort_runs && c->count.rec_n == 0 && c->count.batches == 0 && c->stats_h[ST_CLAIMED] == 0 &&
                !c->count.skm_used && c->runs.empty() && b.n >= direct_min && !test_hook("KC_NO_P5S_DIRECT")) {
                if ((s = part_p5_direct(c, b, nullptr, &dd, &R))) return s;
                if (dd) {
                    c->count.sorted_run_batches++;
                    c->count.hc_hint = R * 2 > b.n;
                    c->count.engines_used |= 2u;
                    done += nr;
                    continue;
                }
            }
            if ((s = sort_runs ? part_p5_sorted(c, b, rec0) : part_p5_hash(c, b, rec0))) return s;
            // the next batch's P5 starts from this one's cardinality
            c->count.hc_hint = (c->count.rec_n - rec0) * 2 > b.n;
            if ((s = flush_spill2(c, b.p5_spill, b.p5_keys))) return s;
        } else if ((s = sync_stats(c))) {
            return s;
        }
        c->count.batches++;
        c->count.engines_used |= 2u;
        // records past half the working set become a sorted run between
        // batches and between passes that did not go direct, as pend_flush
        // does between its calls (a call of many batches or passes must not
        // grow the records past the working set). Not while the next pass's
        // keys wait in fin_packed (two passes per walk), which the cut writes.
        if (!(kpass && kp.u_pass == kp.kpi + 1) && (s = cut_run_if_full(c))) return s;
        if (kpass && kp.kpi + 2 < kp.kp.size()) {
            kp.kpi++;
            continue;
        }
        done += nr;
    }
    c->st.valid_kmers = c->stats_h[ST_VALID];
    c->st.spilled_kmers = c->count.spilled_flushed + c->stats_h[ST_SPILL_FILL];
    return KC_OK;
}

// ---------------------------------------------------------------------------
// Engine "skm" (super-k-mer records; kernels and record layout in kc_skm.inl)
// ---------------------------------------------------------------------------

// Groups n SoA items (NW words at stride sa in `a`, optional u32 payload pa)
// by the 16 bits word0 >> 48: level 1 by bits 48..55 into `b` (writing the
// level-2 digit, bits 56..63, of every item to `digs`), level 2 by bits 56..63
// stable over level 1's regions, back into `a`. ms[0] += histogram + scan
// time, ms[1] += scatter time (HIP events).
kc_status group16(kc_ctx* c, int NW, bool pay, uint64_t* a, uint64_t sa, uint32_t* pa, uint64_t* b, uint64_t sb,
                  uint32_t* pb, uint8_t* digs, uint64_t n, double* ms, const uint8_t* dig1) {
    if (n == 0) return KC_OK;
    kc_status s;
    const uint64_t tile = (uint64_t)rp_tile(NW, pay);
    const uint64_t nt1 = (n + tile - 1) / tile;
    const uint64_t ntmax = nt1 + 256;
    const uint64_t tmpn = rp_tmp_elems(ntmax);
    if ((s = ensure(c, c->part_sort_hist, (256 * ntmax + tmpn + 4 + 2 * 257) * 8))) return s;
    uint64_t* pos = c->part_sort_hist.as<uint64_t>();
    uint64_t* tmp = pos + 256 * ntmax;
    uint64_t* rt = tmp + tmpn;
    const int grid = 2 * c->n_cu;
    Marks mk{c};
    std::vector<uint64_t> h(4 + 2 * 257);
    h[0] = 0;
    h[1] = n;
    h[2] = 0;
    h[3] = nt1;
    HIPCHK(c, hipMemcpyAsync(rt, h.data(), 4 * 8, hipMemcpyHostToDevice, c->stream));
    // (histogram and scatter timed by three marks and the one synchronisation
    // each pass needs anyway: no wait between a histogram and its scatter)
    HIPCHK(c, mk.begin());
    // first pass digit: the producer's byte per item when it wrote one, else word 0 bits 48..55
    const RegionTable reg1 = {rt, rt + 2, 1, nt1, (uint32_t)tile};
    HIPCHK(c, launch_rp_hist(dig1, dig1 ? nullptr : a, 48, reg1, pos, tmp, grid, c->stream));
    HIPCHK(c, mk.mark());
    HIPCHK(c, launch_rp_scatter(NW, pay, a, sa, b, sb, pa, pb, reg1, pos, 48, digs, 56, grid, c->stream));
    HIPCHK(c, mk.mark());
    // level 1's digit bases: level 2's regions
    uint64_t* rs = h.data() + 4;
    HIPCHK(c, hipMemcpyAsync(rs, rp_digit_base(tmp, nt1), 256 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, mk.add(0, ms[0]));
    HIPCHK(c, mk.add(1, ms[1]));
    rs[256] = n;
    const uint64_t nt2 = tile_prefix(rs, 256, tile, rs + 257);
    HIPCHK(c, hipMemcpyAsync(rt + 4, rs, 2 * 257 * 8, hipMemcpyHostToDevice, c->stream));
    const RegionTable reg2 = {rt + 4, rt + 4 + 257, 256, nt2, (uint32_t)tile};
    HIPCHK(c, mk.begin());
    HIPCHK(c, launch_rp_hist(digs, nullptr, 0, reg2, pos, tmp, grid, c->stream));
    HIPCHK(c, mk.mark());
    HIPCHK(c, launch_rp_scatter(NW, pay, b, sb, a, sa, pb, pa, reg2, pos, 56, nullptr, 0, grid, c->stream));
    HIPCHK(c, mk.mark());
    HIPCHK(c, hipEventSynchronize(mk.last()));
    HIPCHK(c, mk.add(0, ms[0]));
    HIPCHK(c, mk.add(1, ms[1]));
    return KC_OK;
}

// Reads of nw windows one skm batch may take beyond key_cap windows (see
// count_reads_skm): the record pool at nw / 4 records per read, while the
// global table is empty; 0 when only safe batches apply
static uint64_t skm_big_reads(const kc_ctx* c, uint64_t nw, uint64_t pool_cap) {
    if (c->count.skm_big_off || c->stats_h[ST_CLAIMED] || c->table_dirty || test_hook("KC_SKM_SAFE_BATCH")) return 0;
    return pool_cap / std::max<uint64_t>(1, nw / 4);
}

// What a batch that may be undone starts from (taken once per batch, after
// sync_stats): the device counters, the record count, and the host-side
// counters, so that kc_stats describes only the work kept
struct BatchSnapshot {
    uint64_t stats[ST_N];
    uint64_t rec_n;
    BatchCounters host;
};

static BatchSnapshot batch_snapshot(const kc_ctx* c) {
    BatchSnapshot b;
    memcpy(b.stats, c->stats_h, sizeof(b.stats));
    b.rec_n = c->count.rec_n;
    b.host = c->count;
    return b;
}

// Undoes a batch: the device counters always, and of the rest what `what` names
enum Undo : unsigned {
    UNDO_HOST = 1,     // the host-side counters
    UNDO_RECORDS = 2,  // the records the batch wrote
    UNDO_TABLE = 4     // the global table, cleared (it was empty before the batch)
};
static kc_status undo_batch(kc_ctx* c, const BatchSnapshot& b, unsigned what) {
    if (what & UNDO_TABLE) HIPCHK(c, hipMemsetAsync(c->table, 0, c->table_bytes, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->stats, b.stats, ST_N * 8, hipMemcpyHostToDevice, c->stream));
    if (what & UNDO_RECORDS) HIPCHK(c, hipMemcpyAsync(c->rec_cursor, &b.rec_n, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(c->stats_h, b.stats, ST_N * 8);
    if (what & UNDO_HOST) static_cast<BatchCounters&>(c->count) = b.host;
    if (what & UNDO_RECORDS) c->count.rec_n = b.rec_n;
    return KC_OK;
}

// One batch of the skm engine, as its stages hand it on
struct SkmBatch {
    CountLaunch l;
    uint64_t pool_cap = 0;    // keys_a / keys_b hold W + 1 x pool_cap record words each
    uint64_t kbound = 0;      // the batch's windows
    bool big = false;         // more than key_cap windows
    uint64_t np = 0;          // F's records (padding included)
    uint8_t* dig1 = nullptr;  // F's first-pass digit bytes
    // P5a (W = 1): each bucket's distinct records written back over the front
    // of its range, multiplicities into the digit bytes (free after S2, read
    // as u32 indexed like the pool); P5 walks them
    bool dedup = false;
    SkmDedup dd = {};
    // P5a's overflow lists (buckets whose distinct records overflow its LDS
    // table, deduplicated again in hash-split passes) go to the pool's free
    // tail: records [over0, over_limit) of keys_a, their multiplicities at the
    // same indices of the digit-byte buffer (u32)
    uint64_t over0 = 0, over_limit = 0;
    // a large batch overflowed the record buffer: it is undone and counted in
    // safe batches like a spill overflow
    bool rec_retry = false;
};

// E + F: the batch's reads into b.np records of the pool (keys_a)
static kc_status skm_front(kc_ctx* c, const SkmGeom& g, int64_t pre0, SkmBatch& b) {
    Marks mk{c};
    HIPCHK(c, hipMemsetAsync(c->pool_cursor, 0, 8, c->stream));
    HIPCHK(c, mk.begin());
    if (pre0 < 0)
        HIPCHK(c, launch_encode_reads(b.l, c->part_codes.as<uint32_t>(), c->part_inval.as<uint16_t>(), c->stream));
    HIPCHK(c, mk.mark());
    HIPCHK(c, hipEventSynchronize(mk.last()));
    HIPCHK(c, mk.add(0, c->count.part_ms[0]));
    HIPCHK(c, mk.begin());
    // digs: the second array (16-byte aligned, for the histogram's 16-byte
    // loads) takes F's first-pass digits, the first the second pass's
    // (written by the first pass)
    const uint64_t dig1_off = (b.pool_cap + 15) & ~15ull;
    b.dig1 = dig1_off + b.pool_cap <= c->digs_bytes ? c->digs + dig1_off : nullptr;
    HIPCHK(c, launch_skm_front(b.l, g, c->keys_a, b.pool_cap, c->pool_cursor, 8 * c->n_cu, c->stream, b.dig1));
    HIPCHK(c, mk.mark());
    HIPCHK(c, hipMemcpyAsync(&b.np, c->pool_cursor, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, mk.add(0, c->count.part_ms[0], c->count.part_ms[1], c->count.insert_ms));
    c->count.insert_launches++;
    return KC_OK;
}

// S1 + S2 + P4: the records grouped by bucket (back in keys_a), the bucket
// bounds in part_starts; then P5a's buffers
static kc_status skm_group(kc_ctx* c, SkmBatch& b) {
    kc_status s;
    const int RW = c->W + 1;
    const uint64_t np = b.np, pool_cap = b.pool_cap;
    Marks mk{c};
    double gm[2] = {0, 0};
    // S's scratch (the first pass's output) at the end of keys_b, at
    // the records' own stride: the radix scatter writes the start of
    // a large allocation ~25% slower than its end in every process
    // measured (tools/rp_bench)
    uint64_t* sbase = c->keys_b;
    uint64_t sbs = pool_cap;
    const uint64_t cs = (np + 255) & ~255ull;
    const uint64_t belems = (uint64_t)RW * pool_cap;
    if ((uint64_t)RW * cs <= belems && !test_hook("KC_S_SCRATCH_START")) {
        sbs = cs;
        sbase = c->keys_b + ((belems - (uint64_t)RW * cs) & ~255ull);
    }
    if ((s = group16(c, RW, false, c->keys_a, pool_cap, nullptr, sbase, sbs, nullptr, c->digs, np, gm, b.dig1)))
        return s;
    c->count.part_ms[3] += gm[0];
    c->count.part_ms[2] += gm[1];
    c->count.part_keys += np;
    const uint32_t nb = 1u << kBucketBits;
    if ((s = ensure(c, c->part_starts, ((size_t)nb + 1) * 8))) return s;
    HIPCHK(c, mk.begin());
    HIPCHK(c, launch_bucket_bounds(1, c->keys_a, pool_cap, np, kBucketBits, c->part_starts.as<uint64_t>(),
                                   c->stream));
    HIPCHK(c, mk.mark());
    HIPCHK(c, hipEventSynchronize(mk.last()));
    HIPCHK(c, mk.add(0, c->count.part_ms[3]));
    b.dedup = c->W == 1 && !test_hook("KC_NO_DEDUP") && np <= c->digs_bytes / 4;
    b.over0 = (np + 63) & ~63ull;
    b.over_limit = std::min<uint64_t>(pool_cap, c->digs_bytes / 4);
    if (const char* e = test_hook("KC_P5A_OVER_ROOM"))  // tests: little room, later buckets stay raw
        b.over_limit = std::min<uint64_t>(b.over_limit, b.over0 + strtoull(e, nullptr, 10));
    const size_t dpos_off = (((size_t)nb + 1) * 4 + 64 + 15) & ~(size_t)15;
    if (b.dedup) {
        if ((s = ensure(c, c->part_dedup, dpos_off + (size_t)nb * 8))) return s;
        b.dd.cnt = c->digs.as<uint32_t>();
        b.dd.len = c->part_dedup.as<uint32_t>();
        b.dd.pos = (const uint64_t*)(c->part_dedup.as<uint8_t>() + dpos_off);
        HIPCHK(c, hipMemcpyAsync(c->pool_cursor, &b.over0, 8, hipMemcpyHostToDevice, c->stream));
    }
    return KC_OK;
}

// P5 over buckets [b0, b1); reruns with a bigger record buffer on overflow
// (safe while nothing went to the global table or spill). A large batch (more
// than key_cap windows) does not grow the buffer to its window count, which
// can be far past the working set: it sets b.rec_retry.
static kc_status skm_p5_range(kc_ctx* c, SkmBatch& b, uint32_t b0, uint32_t b1, bool count_keys) {
    kc_status s;
    const int W = c->W;
    float t = 0.f;
    Marks mk{c};
    uint64_t bound = (uint64_t)(b1 - b0) * (uint64_t)skm_lds_slots(W);
    if (bound > b.kbound) bound = b.kbound;
    if (const char* e = test_hook("KC_P5_REC_BOUND")) {  // tests: force the overflow path
        const uint64_t v = strtoull(e, nullptr, 10);
        if (v > 0 && v < bound) bound = v;
    }
    const uint64_t rec0 = c->count.rec_n;
    const uint64_t claimed0 = c->stats_h[ST_CLAIMED];
    // P5a and P5 back to back, timed by three marks after P5's
    // synchronisation (P5a's time: mark 0 -> 1, P5's: 1 -> 2)
    bool p5a_pending = false;
    if (b.dedup) {
        HIPCHK(c, mk.begin());
        HIPCHK(c, launch_count_rec(c->keys_a, b.pool_cap, c->part_starts.as<uint64_t>(), b0, b1, c->digs.as<uint32_t>(),
                                   c->part_dedup.as<uint32_t>(), c->n_cu, c->stream,
                                   b.over0 < b.over_limit ? c->pool_cursor.as<uint64_t>() : nullptr, b.over_limit,
                                   (uint64_t*)b.dd.pos));
        p5a_pending = true;
    }
    for (;;) {
        if ((s = grow_records(c, rec0 + bound))) return s;
        // keys_b is free after S2: it takes P5's spills (W x key_cap words)
        HIPCHK(c, mk.begin(1));
        HIPCHK(c, launch_count_skm(W, (int)c->k, c->keys_a, b.pool_cap, c->part_starts.as<uint64_t>(), b0, b1,
                                   count_keys, rec_sink(c), p5_fallback(c, c->keys_b, b.l.probe_limit),
                                   c->cfg.lds_slots, c->n_cu, c->stream, b.dedup ? &b.dd : nullptr, c->rec_dig));
        HIPCHK(c, mk.mark());
        HIPCHK(c, hipMemcpyAsync(&c->count.rec_n, c->rec_cursor, 8, hipMemcpyDeviceToHost, c->stream));
        if ((s = sync_stats(c))) return s;
        if (p5a_pending) {
            HIPCHK(c, mk.add(0, c->count.dedup_ms));
            p5a_pending = false;
        }
        HIPCHK(c, mk.ms(1, &t));
        c->count.part_ms[4] += t;
        c->count.p5_launches++;
        if (debug_on())
            fprintf(stderr,
                    "kc: skm F records=%llu P5[%u,%u) passes=%llu aborts=%llu max_m=%llu records=%llu %.3f ms\n",
                    (unsigned long long)b.np, b0, b1, (unsigned long long)c->stats_h[ST_P5_PASSES],
                    (unsigned long long)c->stats_h[ST_P5_ABORTS], (unsigned long long)c->stats_h[ST_P5_MAXM],
                    (unsigned long long)c->count.rec_n, t);
        if (!(c->stats_h[ST_ERR] & ERR_REC_OVERFLOW)) return KC_OK;
        if (b.big) {
            b.rec_retry = true;
            return KC_OK;
        }
        if (bound >= b.kbound || c->stats_h[ST_CLAIMED] != claimed0 || c->stats_h[ST_SPILL2_FILL])
            return fail(c, KC_ERR_INTERNAL, "record buffer overflow");
        bound = b.kbound;
        if ((s = rerun_reset(c, rec0))) return s;
    }
}

// The skm engine's driver: the batch loop over the stages above, the
// cardinality sample, and the undo of a batch that overflowed.
// part_ms slots for this engine: [0] E + F, [1] F, [2] S1/S2 scatters,
// [3] S1/S2 histograms + scans + P4, [4] P5.
static kc_status count_reads_skm(kc_ctx* c, const uint8_t* base, const uint64_t* seq_off, uint64_t n_reads,
                                 int64_t L, const SkmGeom& g, int64_t pre0) {
    if (c->count.finished) return fail(c, KC_ERR_STATE, "kc_finish was called; kc_reset first");
    const int W = c->W;
    const int RW = W + 1;
    const uint64_t nw = (uint64_t)(L - c->k + 1);
    // keys_a / keys_b hold RW x pool_cap record words each; digs holds a byte per record
    uint64_t pool_cap = (uint64_t)W * c->key_cap / RW;
    if (const char* e = test_hook("KC_SKM_POOL_CAP")) {  // tests: force the pool-overflow retry
        const uint64_t v = strtoull(e, nullptr, 10);
        if (v > 0 && v < pool_cap) pool_cap = v;
    }
    // P5's spills go to keys_b (key_cap keys), which a batch of at most
    // key_cap windows can never overflow. While the global table is still
    // empty a batch may be larger, up to what the record pool holds at nw / 4
    // records per read (F's pool-overflow retry catches denser reads): fewer
    // batches, so fewer runs for the finish to merge (SURVEY cfg4: 125M reads
    // per GPU in one batch). A spill overflow in such a batch undoes it (table
    // cleared, records and statistics restored) and retries it at the safe size.
    uint64_t safe_reads = c->key_cap / nw;
    if (safe_reads == 0) return fail(c, KC_ERR_ARG, "gpu_memory_limit too small for one read's windows");
    uint64_t max_reads = std::max(safe_reads, skm_big_reads(c, nw, pool_cap));
    // even batch sizes when a read's code row is an odd number of words: every
    // batch's masks then start 4-byte aligned, which F3's dword DMA needs
    const bool even = (groups_per_read((int)L) & 1) != 0;
    auto even_down = [&](uint64_t v) { return even && v > 1 ? v & ~1ull : v; };
    safe_reads = even_down(safe_reads);
    max_reads = even_down(max_reads);
    kc_status s;
    uint64_t done = 0;
    while (done < n_reads) {
        uint64_t nr = n_reads - done;
        if (nr > max_reads) nr = max_reads;
        if (nr > safe_reads && (c->stats_h[ST_CLAIMED] || c->table_dirty)) {
            nr = safe_reads;  // the table holds keys already: only a safe batch
            max_reads = safe_reads;
        }
        SkmBatch b;
        b.big = nr > safe_reads;
        b.pool_cap = pool_cap;
        b.kbound = nr * nw;
        const uint64_t ng = nr * (uint64_t)groups_per_read((int)L);
        if (pre0 < 0 && ((s = ensure(c, c->part_codes, ng * 4 + 16)) || (s = ensure(c, c->part_inval, ng * 2 + 16))))
            return s;
        b.l = make_launch(c, base, seq_off, done, nr, L, pre0);
        if ((s = sync_stats(c))) return s;
        const BatchSnapshot snap = batch_snapshot(c);
        if ((s = skm_front(c, g, pre0, b))) return s;
        if (b.np > pool_cap) {
            // more records than the pool holds (runs far shorter than usual):
            // undo the batch's statistics and retry with half the reads
            if ((s = undo_batch(c, snap, UNDO_HOST))) return s;
            if (nr <= 1) return fail(c, KC_ERR_INTERNAL, "skm pool overflow on one read");
            max_reads = nr / 2 > 1 ? even_down(nr / 2) : 1;
            continue;
        }
        if (experiment_knob("KC_F_SKIP")) {  // records are invalid, stop after F
            c->count.batches++;
            done += nr;
            continue;
        }
        if (b.np > 0) {
            if ((s = skm_group(c, b))) return s;
            // bucket 0xffff holds only the pool's padding records. Unless this
            // context already knows its data, the first kSkmSample buckets are
            // counted alone: if most of their keys are distinct (iid reads, no
            // coverage) the key-prefix engine takes this batch and the rest,
            // whose sorted finish needs no global sort
            const uint32_t nbk = (1u << kBucketBits) - 1;
            uint32_t bs = 0;
            if (!c->skm_force && !c->count.skm_checked && b.kbound >= kSkmSampleMinKeys) {
                bs = kSkmSample;
                if ((s = skm_p5_range(c, b, 0, bs, true))) return s;
                c->count.skm_checked = true;
                const uint64_t keys_s = c->stats_h[ST_P5_KEYS], dist_s = c->count.rec_n - snap.rec_n;
                if (!b.rec_retry && keys_s > 0 && (double)dist_s > kSkmDistinctMax * (double)keys_s &&
                    c->stats_h[ST_CLAIMED] == snap.stats[ST_CLAIMED] && c->stats_h[ST_SPILL2_FILL] == 0) {
                    // (the host counters stay: the F and S time spent is real)
                    if ((s = undo_batch(c, snap, UNDO_RECORDS))) return s;
                    c->count.skm_hc = true;
                    c->count.hc_hint = true;
                    if (debug_on())
                        fprintf(stderr, "kc: skm sample %llu distinct / %llu keys: key-prefix engine\n",
                                (unsigned long long)dist_s, (unsigned long long)keys_s);
                    return count_reads_part(c, seq_off ? base : base + done * (uint64_t)L,
                                            seq_off ? seq_off + done : nullptr, n_reads - done, L,
                                            pre0 < 0 ? -1 : pre0 + (int64_t)done);
                }
            }
            if (!b.rec_retry && (s = skm_p5_range(c, b, bs, nbk, false))) return s;
            if (b.dedup && !b.rec_retry) {
                HIPCHK(c, launch_dedup_total(c->part_dedup.as<uint32_t>(), c->part_starts.as<uint64_t>(), nbk,
                                             c->stats, c->stream));
                if ((s = sync_stats(c))) return s;
            }
            c->count.skm_used = true;
            c->count.engines_used |= 1u;
            if (((c->stats_h[ST_ERR] & ERR_SPILL_OVERFLOW) || b.rec_retry) && b.big) {
                // undo the large batch and count its reads in safe batches
                if (debug_on())
                    fprintf(stderr, "kc: skm batch of %llu reads overflowed the %s buffer: retried\n",
                            (unsigned long long)nr, b.rec_retry ? "record" : "spill");
                if ((s = undo_batch(c, snap, UNDO_HOST | UNDO_RECORDS | UNDO_TABLE))) return s;
                c->count.skm_big_off = true;
                max_reads = safe_reads;
                continue;
            }
            if ((s = flush_spill2(c, c->keys_b, c->keys_a))) return s;
        } else if ((s = sync_stats(c))) {
            return s;
        }
        c->count.batches++;
        done += nr;
        // a call may span several batches (large batches, or safe ones once
        // the table holds keys): runs are cut between them as between calls
        if (done < n_reads && (s = cut_run_if_full(c))) return s;
    }
    c->st.valid_kmers = c->stats_h[ST_VALID];
    c->st.spilled_kmers = c->count.spilled_flushed + c->stats_h[ST_SPILL_FILL];
    return KC_OK;
}

// Engine choice before the super-k-mer engine's first large batch: the
// coverage sketch of the encoded reads (sketch_k). When most sampled k-mers
// are distinct (low coverage: iid reads, SURVEY cfg5) the key-prefix engine
// counts this batch and the rest of the context's input, and P5 splits its
// buckets up front; the super-k-mer engine's bucket sample (count_reads_skm)
// stays as the second check. Saves the skm engine's F and S passes over a
// batch it would give up.
static const double kSketchDistinctMax = 0.7;
static const double kSketchCoveredMax = 0.6;  // below: the skm bucket sample is not needed

static kc_status sketch_engine(kc_ctx* c, uint64_t n_reads, int64_t L, int64_t pre0) {
    kc_status s;
    const uint64_t G = (uint64_t)groups_per_read((int)L);
    // sample rate 2^-rb by k-mer hash: about 2^18 samples (at least 1/256)
    const uint64_t aligned = n_reads * G;
    int rb = 8;
    while (rb < 24 && (aligned >> rb) > (1ull << 18)) rb++;
    const uint64_t cap = (aligned >> rb) * 2 + 4096;  // twice the expected samples
    // the distinct samples are counted in a set of at least 2 x cap slots
    int set_bits = 1;
    while ((1ull << set_bits) < 2 * cap) set_bits++;
    const size_t set_bytes = ((size_t)8 << set_bits);
    if ((s = ensure(c, c->fin_keys[0], cap * 8 + 64)) || (s = ensure(c, c->fin_keys[1], set_bytes)) ||
        (s = ensure(c, c->fin_misc, 64)))
        return s;
    uint64_t* fp = c->fin_keys[0].as<uint64_t>();
    uint64_t* counter = c->fin_misc.as<uint64_t>();  // [0] samples, [1] distinct samples
    HIPCHK(c, hipMemsetAsync(counter, 0, 16, c->stream));
    HIPCHK(c, hipMemsetAsync(c->fin_keys[1].p, 0, set_bytes, c->stream));
    HIPCHK(c, launch_sketch(c->part_codes.as<uint32_t>() + (uint64_t)pre0 * G,
                            c->part_inval.as<uint16_t>() + (uint64_t)pre0 * G, n_reads, (int)L, (int)c->k, rb, fp,
                            cap, counter, c->stream));
    HIPCHK(c, launch_sketch_distinct(fp, counter, cap, c->fin_keys[1].as<uint64_t>(), set_bits, counter + 1, c->stream));
    uint64_t md[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(md, counter, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t m = md[0];
    if (m > cap) m = cap;
    if (m < 4096) return KC_OK;  // too few samples to tell: the skm engine's own sample decides
    const uint64_t distinct = md[1];
    if (debug_on())
        fprintf(stderr, "kc: sketch %llu distinct / %llu sampled k-mers\n", (unsigned long long)distinct,
                (unsigned long long)m);
    if ((double)distinct > kSketchDistinctMax * (double)m) {
        c->count.skm_hc = true;
        c->count.hc_hint = true;
        c->count.skm_checked = true;
    } else if ((double)distinct < kSketchCoveredMax * (double)m && !test_hook("KC_SKM_SAMPLE")) {
        // clear coverage: the skm engine's bucket sample (its own check, at
        // 35% distinct keys) would keep the skm engine too; skipped, which
        // saves its two small launches and their synchronisation. (The sketch
        // samples only 16-base-aligned positions, so a k-mer covered c times
        // is sampled ~c/16 times: 60% distinct samples is a window coverage of
        // ~16, where about 6% of the keys are distinct)
        c->count.skm_checked = true;
    }
    return KC_OK;
}

// The coverage sketch picks the engine (auto) or, for the partition engine,
// sets the high-cardinality hint before its first batch
static kc_status sketch_gate(kc_ctx* c, uint64_t n_reads, int64_t L, int64_t pre0) {
    const bool skm_ok = skm_geometry((int)L, (int)c->k).ok;
    const bool sketch_skm = c->skm && !c->count.skm_hc && !c->skm_force && skm_ok;
    // (the key-prefix engine: chosen, or the default engine's only one for this (L, k))
    const bool sketch_part = c->part && !c->count.hc_hint && !(c->skm && !c->count.skm_hc && skm_ok);
    if ((sketch_skm || sketch_part) && !c->count.skm_checked && pre0 >= 0 && !test_hook("KC_NO_SKETCH") &&
        n_reads * (uint64_t)(L - c->k + 1) >= kSkmSampleMinKeys) {
        kc_status s = sketch_engine(c, n_reads, L, pre0);
        if (s) return s;
        if (sketch_part) c->count.skm_checked = true;  // once per reset
    }
    return KC_OK;
}

// pre0 >= 0: the reads are pre-encoded in part_codes / part_inval from read pre0
static kc_status count_reads(kc_ctx* c, const uint8_t* base, const uint64_t* seq_off, uint64_t n_reads, int64_t L,
                             int64_t pre0 = -1) {
    kc_status s0 = sketch_gate(c, n_reads, L, pre0);
    if (s0) return s0;
    // very long reads (one read's windows do not fit a P2 workgroup's LDS)
    // take the table engine; both feed the same finish
    if (c->skm && !c->count.skm_hc) {
        const SkmGeom g = skm_geometry((int)L, (int)c->k);
        if (g.ok) return count_reads_skm(c, base, seq_off, n_reads, L, g, pre0);
    }
    if (c->part && part_geometry((int)L, (int)c->k, 1).lds_scatter <= kMaxLds)
        return count_reads_part(c, base, seq_off, n_reads, L, pre0);
    if (pre0 >= 0) return fail(c, KC_ERR_INTERNAL, "pre-encoded reads reached the table engine");
    return count_reads_table(c, base, seq_off, n_reads, L);
}

// ---------------------------------------------------------------------------
// pending batch (see kc_ctx::pend_*)
// ---------------------------------------------------------------------------

// Reads of length L one engine batch holds (its window capacity key_cap)
static uint64_t batch_reads(const kc_ctx* c, int64_t L) {
    const uint64_t m = c->key_cap / (uint64_t)(L - c->k + 1);
    return m ? m : 1;
}

// Pending reads of length L allowed before a flush. While a checkpoint is held
// the batch may grow past one engine batch (count_reads splits it) up to
// 1/8 of the device's memory in codes (6 B per 16 bases), so a malformed block
// later in the same file can still be rolled back.
// Without a checkpoint the codes engines still pend up to 16 engine batches
// (within the same budget): a high-cardinality batch is then counted in
// key-range passes over all its reads instead of read batches whose runs must
// be merged (count_reads_part).
static uint64_t pend_room(const kc_ctx* c, int64_t L, bool var = false) {
    const uint64_t b = batch_reads(c, L);
    if (!c->count.ckpt && (!c->part || var)) return b;
    const uint64_t per_read = 6 * (uint64_t)groups_per_read((int)L) + 2;
    uint64_t budget = c->dev_total / 8 / per_read;
    if (!c->count.ckpt && budget / 16 > b) budget = 16 * b;
    return budget > b ? budget : b;
}

// Grows b to at least `bytes`, keeping its first `keep` bytes.
static kc_status grow_keep(kc_ctx* c, DevBuf& b, size_t bytes, size_t keep) {
    if (b.p && b.bytes >= bytes) return KC_OK;
    size_t want = bytes < 256 ? 256 : bytes;
    if (b.p && want < b.bytes + b.bytes / 2) want = b.bytes + b.bytes / 2;
    DevBuf nb;
    HIPCHK(c, nb.alloc(want));
    if (b.p && keep) HIPCHK(c, hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b = std::move(nb);
    return KC_OK;
}

// Counts the pending batch (the engines: count_reads with pre-encoded reads).
extern "C" {
static kc_status chunk_acc_flush(kc_ctx* c);  // defined with the chunk entry points (C linkage block)
}

// Key 0's presence for reads whose slots hold positions that are no bases
// (variable-length padding, one-pass empty rows): the engines read those as
// not-ACGT, so it is recomputed as (presence before the flush) | ST_VHOLE (a
// read of >= k bases holds a not-ACGT base, set by the encoders) | a key-0
// window counted. Also applied before a run is cut inside such a flush.
kc_status recompute_presence(kc_ctx* c) {
    kc_status s;
    if ((s = sync_stats(c))) return s;
    const uint64_t present =
        (c->flush_present0 | c->stats_h[ST_VHOLE] | (c->stats_h[ST_KEY0] != 0 ? 1u : 0u)) ? 1u : 0u;
    c->stats_h[ST_KEY0_PRESENT] = present;
    HIPCHK(c, hipMemcpyAsync(c->stats + ST_KEY0_PRESENT, &c->stats_h[ST_KEY0_PRESENT], 8, hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KC_OK;
}

// Fixed-length pending reads [0, n): more than one engine batch is counted
// whole when it is a high-cardinality batch on an empty record state
// (key-range passes, count_reads_part), anything else batch by batch with a
// run cut between batches when the records outgrow half the working set
static kc_status pend_count_fixed(kc_ctx* c, uint64_t n) {
    kc_status s;
    const int64_t L = c->count.pend_L;
    const uint64_t b = batch_reads(c, L);
    if (n > b) {
        if ((s = sketch_gate(c, n, L, 0))) return s;
        const bool passes = c->count.hc_hint && c->part && (!c->skm || c->count.skm_hc) && c->count.rec_n == 0 && c->count.batches == 0 &&
                            !c->count.skm_used && c->runs.empty() && !test_hook("KC_NO_KEY_PASSES");
        if (!passes) {
            // the skm engine may take a large batch (count_reads_skm)
            uint64_t bs = b;
            if (c->skm && !c->count.skm_hc && skm_geometry((int)L, (int)c->k).ok) {
                const uint64_t nw = (uint64_t)(L - c->k + 1);
                bs = std::max(b, skm_big_reads(c, nw, (uint64_t)c->W * c->key_cap / (c->W + 1)));
            }
            // (an even read count per slice when a code row has an odd number
            // of words: each slice's masks start 4-byte aligned for F3)
            if ((groups_per_read((int)L) & 1) && bs > 1) bs &= ~1ull;
            for (uint64_t r0 = 0; r0 < n; r0 += bs) {
                if ((s = count_reads(c, nullptr, nullptr, n - r0 < bs ? n - r0 : bs, L, (int64_t)r0))) return s;
                if ((s = cut_run_if_full(c))) return s;
            }
            return KC_OK;
        }
    }
    if ((s = count_reads(c, nullptr, nullptr, n, L, 0))) return s;
    return cut_run_if_full(c);
}

kc_status pend_flush(kc_ctx* c) {
    if (c->count.acc_n) {
        kc_status s0 = chunk_acc_flush(c);
        if (s0) return s0;
    }
    if (c->count.pend_reads == 0) return KC_OK;
    kc::trace("flush %llu reads of length %lld", (unsigned long long)c->count.pend_reads, (long long)c->count.pend_L);
    const uint64_t n = c->count.pend_reads;
    c->count.pend_reads = 0;  // a failed count is not counted again
    c->flushes++;
    const bool sparse = c->count.pend_sparse;
    c->count.pend_sparse = false;
    if (!c->count.pend_var && !sparse) return pend_count_fixed(c, n);
    // variable-length reads (slot padding) or one-pass rows (empty rows): the
    // skm front end reads each row's length; key 0's presence is recomputed
    kc_status s;
    if ((s = sync_stats(c))) return s;
    c->flush_present0 = c->stats_h[ST_KEY0_PRESENT];
    c->var_rlen = c->part_rlen.as<uint16_t>();
    s = c->count.pend_var ? count_reads(c, nullptr, nullptr, n, c->count.pend_L, 0) : pend_count_fixed(c, n);
    c->var_rlen = nullptr;
    if (s) return s;
    if ((s = recompute_presence(c))) return s;
    return c->count.pend_var ? cut_run_if_full(c) : KC_OK;
}

// Room for n_new more pending reads of length L (fixed or variable): the
// pending batch is counted first when it is of another kind or n_new would
// not fit; the buffers grow keeping the pending reads. *off receives the
// read index where the new reads go.
static kc_status pend_reserve(kc_ctx* c, int64_t L, bool var, uint64_t n_new, uint64_t* off, bool sparse = false) {
    kc_status s;
    if (c->count.pend_reads && (c->count.pend_L != L || c->count.pend_var != var || c->count.pend_reads + n_new > pend_room(c, L, var)))
        if ((s = pend_flush(c))) return s;
    const uint64_t G = (uint64_t)groups_per_read((int)L);
    const uint64_t keep = c->count.pend_reads * G, need = (c->count.pend_reads + n_new) * G;
    if ((s = grow_keep(c, c->part_codes, need * 4 + 16, keep * 4)) ||
        (s = grow_keep(c, c->part_inval, need * 2 + 16, keep * 2)))
        return s;
    if ((var || sparse || c->count.pend_sparse) &&
        (s = grow_keep(c, c->part_rlen, (c->count.pend_reads + n_new) * 2 + 16, c->count.pend_reads * 2)))
        return s;
    // a one-pass block joins reads of full length L: their lengths first
    if (sparse && !c->count.pend_sparse && c->count.pend_reads)
        HIPCHK(c, hipMemsetD16Async((hipDeviceptr_t)c->part_rlen.p, (unsigned short)L, c->count.pend_reads, c->stream));
    c->count.pend_L = L;
    c->count.pend_var = var;
    *off = c->count.pend_reads;
    return KC_OK;
}

// Encodes n_reads reads of device text into the pending batch, one engine
// batch at a time (kernel E): reads at r * L (reference chunks, seq_off null)
// or at seq_off[r] (variable-length: up to seq_end[r], padded slots).
static kc_status pend_add_reads(kc_ctx* c, const uint8_t* base, const uint64_t* seq_off, const uint64_t* seq_end,
                                uint64_t n_reads, int64_t L, bool var) {
    kc_status s;
    const uint64_t G = (uint64_t)groups_per_read((int)L);
    uint64_t done = 0;
    while (done < n_reads) {
        uint64_t free = 0;
        if (c->count.pend_L == L && c->count.pend_var == var && c->count.pend_reads < pend_room(c, L, var))
            free = pend_room(c, L, var) - c->count.pend_reads;
        if (free == 0 || c->count.pend_reads == 0) free = pend_room(c, L, var);
        const uint64_t m = n_reads - done < free ? n_reads - done : free;
        uint64_t off = 0;
        if ((s = pend_reserve(c, L, var, m, &off))) return s;
        uint32_t* codes = c->part_codes.as<uint32_t>() + off * G;
        uint16_t* inval = c->part_inval.as<uint16_t>() + off * G;
        if (var) {
            HIPCHK(c, launch_encode_reads_var(base, seq_off + done, seq_end + done, m, (int)L, (int)c->k, codes, inval,
                                              c->part_rlen.as<uint16_t>() + off, c->stats, c->stream));
        } else {
            const CountLaunch l = make_launch(c, base, seq_off, done, m, L, -1);
            HIPCHK(c, launch_encode_reads(l, codes, inval, c->stream, c->stats));
            if (c->count.pend_sparse)  // rows of a one-pass batch carry their length
                HIPCHK(c, hipMemsetD16Async((hipDeviceptr_t)(c->part_rlen.as<uint16_t>() + off), (unsigned short)L, m,
                                            c->stream));
        }
        c->count.pend_reads += m;
        done += m;
    }
    return KC_OK;
}

// The engine count_reads takes for L reads (same order of tests): the skm and
// key-prefix engines read 2-bit codes, the table engine the text
static bool engine_reads_codes(const kc_ctx* c, int64_t L) {
    if (c->skm && !c->count.skm_hc && skm_geometry((int)L, (int)c->k).ok) return true;
    return c->part && part_geometry((int)L, (int)c->k, 1).lds_scatter <= kMaxLds;
}

// K1 for one record-aligned FASTQ block in device memory (GPU FASTQ decode,
// replacing FASTQFileReader::readData, FASTQFileReader.cpp:49-89): newline
// counts per 16 KiB chunk -> each chunk's first line index -> one of
//   fused   : index + checks + 2-bit encode in one read of the text, straight
//             into the pending batch (fq_encode_k; fq_encode_k<true> for
//             variable-length reads), when the block fits the pending room;
//   two-pass: sequence offsets (fq_emit_k) + length check (fq_validate_k),
//             then encode per batch (kernel E) — blocks larger than a batch,
//             and the table engine, which counts the text itself.
// The whole block is checked before any of its reads is pending or counted: a
// malformed block changes nothing and returns KC_ERR_FORMAT. With count =
// false only the checks run (kc_check_fastq).
static std::string fq_errors(uint64_t e, bool var) {
    std::string why;
    if (e & ERR_FQ_NOT_AT) why += " record-does-not-start-with-@";
    if (e & ERR_FQ_NO_PLUS) why += " no-+-line-after-sequence";
    if (e & ERR_FQ_SEQ_LEN) why += var ? " sequence-longer-than-L" : " sequence-length-differs-from-L";
    if (e & ERR_FQ_TOO_MANY) why += " index-overflow";
    if (e & ERR_FQ_NO_FINAL_NL) why += " block-does-not-end-with-newline";
    return why;
}

static kc_status ingest_fastq(kc_ctx* c, const uint8_t* base, uint64_t n, int64_t L, bool var, bool count,
                              uint64_t* n_rec_out, bool two_pass = false, bool no_spec = false) {
    kc_status s;
    uint64_t nch = fq_chunks(base, n);
    if ((s = ensure(c, c->fq_counts, nch * 8 + 16)) || (s = ensure(c, c->fq_base, nch * 8)) ||
        (s = ensure(c, c->fq_tmp, scan_tmp_elems(nch) * 8)))
        return s;
    if ((s = sync_stats(c))) return s;
    uint64_t snap[ST_N];
    memcpy(snap, c->stats_h, sizeof(snap));
    auto restore = [&]() -> kc_status {
        // the counters the index / encode kernels touched (errors, variable-length hole flag and windows)
        snap[ST_ERR] = 0;
        HIPCHK(c, hipMemcpyAsync(c->stats, snap, sizeof(snap), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        memcpy(c->stats_h, snap, sizeof(snap));
        return KC_OK;
    };
    // One-pass index (fixed L, codes engines): the text is read once; every
    // chunk guesses its line phase and writes its records to rows of its own,
    // then the guesses are checked against the scanned newline counts. A miss
    // or any error: the block is indexed again by the path below, which also
    // gives format errors their verdict.
    // Only where the super-k-mer engine's F3 front end will read the rows (it
    // skips an empty row for free): the key-prefix front end walks them
    // (cfg5, k = 55: P1 + P2 +1.5 ms against 0.7 ms saved in the index,
    // same-box A/B), as do F2 and the W >= 2 front ends
    // (the same conditions as F3's own choice: skm engine not
    // handed over to the key-prefix engine, F3's geometry and LDS budget)
    const bool f3_rows = c->skm && !c->count.skm_hc && c->W == 1 && c->k >= 19 && c->k <= 32 &&
                         skm_f3_applies((int)L, (int)c->k);
    const bool spec = count && !var && !two_pass && !no_spec && f3_rows && engine_reads_codes(c, L) &&
                      fq_spec_ok((int)L) && !test_hook("KC_NO_FQ_ENCODE") && !test_hook("KC_NO_FQ_SPEC");
    const uint64_t spec_rows = spec ? nch * fq_spec_rows_per_chunk((int)L) : 0;
    if (spec && spec_rows <= pend_room(c, L)) {
        uint64_t off = 0;
        if ((s = pend_reserve(c, L, false, spec_rows, &off, true)) || (s = ensure(c, c->fq_phase, nch + 16)))
            return s;
        const uint64_t G = (uint64_t)groups_per_read((int)L);
        Marks mk{c};
        HIPCHK(c, mk.begin());
        HIPCHK(c, hipMemsetAsync(c->stats + ST_ERR, 0, 8, c->stream));
        HIPCHK(c, launch_fq_encode_spec(base, n, (int)L, c->part_codes.as<uint32_t>() + off * G,
                                        c->part_inval.as<uint16_t>() + off * G, c->part_rlen.as<uint16_t>() + off,
                                        c->fq_counts.as<uint64_t>(), c->fq_phase.as<uint8_t>(), c->stats, c->stream));
        HIPCHK(c, launch_scan_u64(c->fq_counts.as<uint64_t>(), c->fq_base.as<uint64_t>(), nch, c->fq_tmp.as<uint64_t>(),
                                  c->stream));
        HIPCHK(c, launch_fq_spec_verify(c->fq_base.as<uint64_t>(), c->fq_phase.as<uint8_t>(), nch, c->stats,
                                        c->stream));
        // [nch]: the line total; [nch + 1]: the rows per chunk the kernel used
        uint64_t* total = c->fq_counts.as<uint64_t>() + nch;
        HIPCHK(c, launch_sum_last(c->fq_base.as<uint64_t>(), c->fq_counts.as<uint64_t>(), nch, total, c->stream));
        uint64_t lr[2] = {0, 0};
        HIPCHK(c, hipMemcpyAsync(lr, total, 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, mk.mark());
        if ((s = sync_stats(c))) return s;
        HIPCHK(c, mk.add(0, c->st.decode_ms));
        const uint64_t lines = lr[0];
        if (c->stats_h[ST_ERR] == 0 && lines % 4 == 0 && lines > 0 && lr[1] >= 1 &&
            lr[1] <= fq_spec_rows_per_chunk((int)L)) {
            const uint64_t n_rec = lines / 4;
            if (n_rec_out) *n_rec_out = n_rec;
            // rows the kernel used (<= the reserved spec_rows). The pending
            // batch counts rows, empty ones included (~4% at cfg2's headers, up
            // to ~15% for short headers): batch sizing, the record pool's
            // reservation and the sketch's sampling rate treat every row as a
            // read, so they err on the safe side (more room reserved, a few
            // more samples); st.reads and st.windows count the real records
            c->count.pend_reads += nch * lr[1];
            c->count.pend_sparse = true;
            c->st.reads += n_rec;
            c->st.windows += n_rec * (uint64_t)(L - c->k + 1);
            return KC_OK;
        }
        if (debug_on())
            fprintf(stderr, "kc: one-pass FASTQ index missed (errors %#llx, %llu lines): two-kernel index\n",
                    (unsigned long long)c->stats_h[ST_ERR], (unsigned long long)lines);
        if ((s = restore())) return s;
        return ingest_fastq(c, base, n, L, var, count, n_rec_out, false, true);
    }
    Marks mk{c};
    HIPCHK(c, mk.begin());
    HIPCHK(c, hipMemsetAsync(c->stats + ST_ERR, 0, 8, c->stream));
    HIPCHK(c, launch_fq_count(base, n, c->fq_counts.as<uint64_t>(), c->stream));
    HIPCHK(c, launch_scan_u64(c->fq_counts.as<uint64_t>(), c->fq_base.as<uint64_t>(), nch, c->fq_tmp.as<uint64_t>(),
                              c->stream));
    // the line count (last chunk's base + count, summed on the device: one readback)
    uint64_t* total = c->fq_counts.as<uint64_t>() + nch;
    HIPCHK(c, launch_sum_last(c->fq_base.as<uint64_t>(), c->fq_counts.as<uint64_t>(), nch, total, c->stream));
    uint64_t lines = 0;
    HIPCHK(c, hipMemcpyAsync(&lines, total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (lines % 4 != 0)
        return fail(c, KC_ERR_FORMAT, "FASTQ block has %llu lines, not a multiple of 4", (unsigned long long)lines);
    const uint64_t n_rec = lines / 4;
    const uint64_t G = (uint64_t)groups_per_read((int)L);
    const bool codes = engine_reads_codes(c, L);
    if (var && (!c->part || !codes))
        return fail(c, KC_ERR_ARG, "variable-length reads need an engine that reads encoded reads (L = %lld)",
                    (long long)L);
    // where the block's reads go: the pending batch when they fit it (after
    // counting a pending batch of another kind or too full to take them)
    uint64_t off = 0;
    // (count = false, kc_check_fastq: the two-pass index checks the block and
    // nothing is reserved, encoded or flushed: a validation has no side effects)
    const bool into_pend = count && codes && n_rec > 0 && n_rec <= pend_room(c, L, var);
    if (into_pend && (s = pend_reserve(c, L, var, n_rec, &off))) return s;
    const bool no_fuse = test_hook("KC_NO_FQ_ENCODE") != nullptr;  // path selector (tests): same bytes either way
    const bool fused = into_pend && !var && !no_fuse;                               // fq_encode_k
    const bool whole_var = into_pend && var;                                         // the block encoded whole
    const bool fused_var = whole_var && !two_pass && !no_fuse && fq_encode_var_ok((int)L);  // fq_encode_k<true>
    if (fused) {
        HIPCHK(c, launch_fq_encode(base, n, c->fq_base.as<uint64_t>(), n_rec, (int)L,
                                   c->part_codes.as<uint32_t>() + off * G, c->part_inval.as<uint16_t>() + off * G,
                                   c->stats, c->stream));
    } else if (fused_var) {
        HIPCHK(c, launch_fq_encode_var(base, n, c->fq_base.as<uint64_t>(), n_rec, (int)L, (int)c->k,
                                       c->part_codes.as<uint32_t>() + off * G, c->part_inval.as<uint16_t>() + off * G,
                                       c->part_rlen.as<uint16_t>() + off, c->stats, c->stream));
    } else {
        if ((s = ensure(c, c->seq_off, n_rec * 8 + 8)) || (s = ensure(c, c->seq_end, n_rec * 8 + 8))) return s;
        HIPCHK(c, launch_fq_emit(base, n, c->fq_base.as<uint64_t>(), c->seq_off.as<uint64_t>(), c->seq_end.as<uint64_t>(),
                                 n_rec, c->stats, c->stream));
        HIPCHK(c, launch_fq_validate(c->seq_off.as<uint64_t>(), c->seq_end.as<uint64_t>(), n_rec, (int)L, c->stats,
                                     c->stream, var));
        if (whole_var)
            HIPCHK(c, launch_encode_reads_var(base, c->seq_off.as<uint64_t>(), c->seq_end.as<uint64_t>(),
                                              n_rec, (int)L, (int)c->k, c->part_codes.as<uint32_t>() + off * G,
                                              c->part_inval.as<uint16_t>() + off * G, c->part_rlen.as<uint16_t>() + off,
                                              c->stats, c->stream));
    }
    HIPCHK(c, mk.mark());
    if ((s = sync_stats(c))) return s;
    HIPCHK(c, mk.add(0, c->st.decode_ms));
    const uint64_t e = c->stats_h[ST_ERR];
    if (fused_var && (e & ERR_FQ_LIST)) {
        // a half held more records than the fused list: the two-pass index
        if ((s = restore())) return s;
        return ingest_fastq(c, base, n, L, var, count, n_rec_out, true, no_spec);
    }
    if (e) {
        const std::string why = fq_errors(e, var);
        if ((s = restore())) return s;
        return fail(c, KC_ERR_FORMAT, "FASTQ block is not 4-line records with %s%lld-base reads:%s",
                    var ? "at most " : "", (long long)L, why.c_str());
    }
    if (n_rec_out) *n_rec_out = n_rec;
    if (!count) return var ? restore() : KC_OK;  // (the encoded reads past pend_reads are dropped)
    const uint64_t vwin0 = snap[ST_VWIN];
    c->st.reads += n_rec;
    if (fused || whole_var) {
        if (fused && c->count.pend_sparse)  // rows of a one-pass batch carry their length
            HIPCHK(c, hipMemsetD16Async((hipDeviceptr_t)(c->part_rlen.as<uint16_t>() + off), (unsigned short)L, n_rec,
                                        c->stream));
        c->count.pend_reads += n_rec;
    } else if (codes) {
        if ((s = pend_add_reads(c, base, c->seq_off.as<uint64_t>(), c->seq_end.as<uint64_t>(), n_rec, L, var)))
            return s;
    } else {
        // the table engine reads the text: counted now
        if ((s = pend_flush(c))) return s;
        if ((s = count_reads(c, base, c->seq_off.as<uint64_t>(), n_rec, L))) return s;
    }
    if (var) {
        if ((s = sync_stats(c))) return s;
        c->st.windows += c->stats_h[ST_VWIN] - vwin0;  // the reads' own windows, not the padded slots'
    } else {
        c->st.windows += n_rec * (uint64_t)(L - c->k + 1);
    }
    return KC_OK;
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" {

int32_t kc_abi_version(void) { return KC_ABI_VERSION; }

int32_t kc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* kc_strerror(kc_status s) {
    switch (s) {
    case KC_OK: return "ok";
    case KC_ERR_ARG: return "invalid argument";
    case KC_ERR_HIP: return "HIP runtime error";
    case KC_ERR_NOMEM: return "out of memory";
    case KC_ERR_FORMAT: return "malformed FASTQ block";
    case KC_ERR_IO: return "I/O error";
    case KC_ERR_STATE: return "invalid call for the context state";
    case KC_ERR_NODEVICE: return "no HIP device";
    case KC_ERR_INTERNAL: return "internal error";
    }
    return "unknown status";
}

const char* kc_last_error(const kc_ctx* c) { return c ? c->err.c_str() : ""; }

kc_status kc_create(kc_ctx** out, const kc_config* cfg) {
    if (!out || !cfg) return KC_ERR_ARG;
    *out = nullptr;
    if (cfg->kmer_length < 1 || cfg->kmer_length > KC_MAX_K) return KC_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return KC_ERR_NODEVICE;
    if (cfg->device < 0 || cfg->device >= ndev) return KC_ERR_NODEVICE;
    kc_ctx* c = new kc_ctx();
    c->cfg = *cfg;
    c->temp_dir = (cfg->temp_dir && cfg->temp_dir[0]) ? cfg->temp_dir : "";
    c->cfg.temp_dir = nullptr;
    c->k = cfg->kmer_length;
    c->W = (int)((c->k + 31) / 32);
    c->rs = 8 * c->W + 4;
    c->id = g_ctx_seq.fetch_add(1);
    memset(&c->st, 0, sizeof(c->st));
    kc_status s = KC_OK;
    auto bail = [&](kc_status e) {
        kc_destroy(c);
        return e;
    };
    if (hipSetDevice(cfg->device) != hipSuccess) return bail(KC_ERR_NODEVICE);
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return bail(KC_ERR_HIP);
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreate(&c->ev2) != hipSuccess || hipEventCreate(&c->evf[0]) != hipSuccess ||
        hipEventCreate(&c->evf[1]) != hipSuccess)
        return bail(KC_ERR_HIP);
    uint64_t M = cfg->gpu_memory_limit ? cfg->gpu_memory_limit : 100000000ull;
    if (M < (1u << 20)) M = 1u << 20;
    // (the table engine reads the text, not encoded reads)
    if ((cfg->flags & KC_FLAG_VARLEN) && (cfg->flags & KC_FLAG_ENGINE_TABLE)) return bail(KC_ERR_ARG);
    c->part = (cfg->flags & KC_FLAG_ENGINE_TABLE) == 0;
    c->skm = c->part && (cfg->flags & KC_FLAG_ENGINE_PREFIX) == 0;
    c->skm_force = (cfg->flags & KC_FLAG_ENGINE_SKM) != 0;
    size_t slot_bytes = 8 * (size_t)slot_words(c->W);
    size_t spill_bytes, tbytes;
    if (c->part) {
        // partition engine: two key buffers take the working set; the global
        // table and spill buffer only catch LDS-table overflow
        spill_bytes = M / 64;
        tbytes = cfg->table_bytes ? cfg->table_bytes : M / 16;
        uint64_t rest = M - M / 64 - M / 16;
        c->key_cap = rest / (16 * (uint64_t)c->W + 1);  // two key buffers + the P3 digit byte
        if (c->key_cap < 65536) c->key_cap = 65536;
    } else {
        spill_bytes = M / 16;
        tbytes = cfg->table_bytes ? cfg->table_bytes : (M - 4 * spill_bytes);
    }
    c->spill_cap = spill_bytes / (8 * c->W);
    if (c->spill_cap < 4096) c->spill_cap = 4096;
    c->cap = tbytes / slot_bytes;
    if (c->cap < 1024) c->cap = 1024;
    c->table_bytes = c->cap * slot_bytes;
    if (c->table.alloc(c->table_bytes) != hipSuccess) return bail(KC_ERR_NOMEM);
    if (c->spill.alloc((size_t)c->spill_cap * 8 * c->W) != hipSuccess) return bail(KC_ERR_NOMEM);
    if (c->stats.alloc(ST_N * 8) != hipSuccess) return bail(KC_ERR_NOMEM);
    if (hipHostMalloc((void**)&c->stats_h, ST_N * 8, 0) != hipSuccess) return bail(KC_ERR_NOMEM);
    if (c->part) {
        if (c->keys_a.alloc((size_t)c->key_cap * 8 * c->W) != hipSuccess) return bail(KC_ERR_NOMEM);
        if (c->keys_b.alloc((size_t)c->key_cap * 8 * c->W) != hipSuccess) return bail(KC_ERR_NOMEM);
        // key_cap digit bytes for the partition engine; the skm engine's two digit
        // arrays (2 x pool_cap, pool_cap = W key_cap / (W + 1)) with the second one
        // 16-byte aligned
        c->digs_bytes = c->key_cap;
        const uint64_t pool_max = (uint64_t)c->W * c->key_cap / (c->W + 1);
        if (((pool_max + 15) & ~15ull) + pool_max > c->digs_bytes) c->digs_bytes = ((pool_max + 15) & ~15ull) + pool_max;
        if (c->digs.alloc((size_t)c->digs_bytes + 16) != hipSuccess) return bail(KC_ERR_NOMEM);
        if (c->rec_cursor.alloc(8) != hipSuccess) return bail(KC_ERR_NOMEM);
        if (c->pool_cursor.alloc(8) != hipSuccess) return bail(KC_ERR_NOMEM);
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0)
            c->n_cu = prop.multiProcessorCount;
    }
    size_t mfree = 0, mtotal = 0;
    if (hipMemGetInfo(&mfree, &mtotal) == hipSuccess) c->dev_total = mtotal;
    s = kc_reset(c);
    if (s) return bail(s);
    *out = c;
    return KC_OK;
}

// Ordered teardown of what is not a device buffer; the buffers go with the
// context object (every stream has been synchronised by then).
void kc_destroy(kc_ctx* c) {
    if (!c) return;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c->ring;  // waits for its DMAs
    delete c->pool;
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    for (char* b : c->file_bufs) (void)hipHostFree(b);
    for (char* b : c->acc_buf)
        if (b) (void)hipHostFree(b);
    if (c->stats_h) (void)hipHostFree(c->stats_h);
    for (auto* evs : {&c->acc_ev, &c->file_ev, &c->stage_free, &c->evf})
        for (hipEvent_t e : *evs)
            if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {c->ev0, c->ev1, c->ev2})
        if (e) (void)hipEventDestroy(e);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    for (auto& r : c->runs)
        if (!r.path.empty()) unlink(r.path.c_str());
    delete c;
}

kc_status kc_reset(kc_ctx* c) {
    if (!c) return KC_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // the global table is cleared only when a slot was claimed since the last
    // clear (the partition engine's table is a rarely used fallback: clearing
    // 1/16 of gpuMemoryLimit per reset would cost milliseconds per count)
    kc_status s0 = sync_stats(c);
    if (s0) return s0;
    if (c->table_dirty || c->stats_h[ST_CLAIMED] > 0) {
        HIPCHK(c, hipMemsetAsync(c->table, 0, c->table_bytes, c->stream));
        c->table_dirty = false;
    }
    HIPCHK(c, hipMemsetAsync(c->stats, 0, ST_N * 8, c->stream));
    if (c->rec_cursor) HIPCHK(c, hipMemsetAsync(c->rec_cursor, 0, 8, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memset(c->stats_h, 0, ST_N * 8);
    // (acc_n: a DMA still reading an accumulation buffer is waited for before it is refilled)
    c->count = CountState();
    for (auto& r : c->runs)
        if (!r.path.empty()) unlink(r.path.c_str());
    c->runs.clear();
    release_dev_runs(c);
    memset(&c->st, 0, sizeof(c->st));
    c->st.table_capacity = c->cap;
    return KC_OK;
}

// Host staging (pinned ring + copy pool), created on first use.
static kc_status stage_init(kc_ctx* c) {
    if (!c->pool) {
        // host copy threads: the CPUs this process may run on, at most 16 (the
        // GPU box's cgroup quota; its affinity mask shows every core)
        cpu_set_t cs;
        int n = 8;
        if (sched_getaffinity(0, sizeof(cs), &cs) == 0) n = CPU_COUNT(&cs);
        c->pool = new kc::Pool(std::max(2, std::min(16, n)));
    }
    if (!c->ring) {
        c->ring = new kc::PinnedRing();
        HIPCHK(c, c->ring->init((size_t)64 << 20, 4));
    }
    return KC_OK;
}

// Reference-exact chunk in device memory: floor(size / L) reads at stride L
// (GPUHandler.cu:13-15), encoded into the pending batch (codes engines) or
// counted from the text (table engine).
static kc_status chunk_device(kc_ctx* c, const uint8_t* d, int64_t size, int64_t L, bool add_stats = true) {
    if (c->count.finished) return fail(c, KC_ERR_STATE, "kc_finish was called; kc_reset first");
    const uint64_t n = (uint64_t)(size / L);
    if (n == 0) return KC_OK;
    kc_status s;
    if (engine_reads_codes(c, L)) {
        if ((s = pend_add_reads(c, d, nullptr, nullptr, n, L, false))) return s;
    } else {
        if ((s = pend_flush(c))) return s;
        if ((s = count_reads(c, d, nullptr, n, L))) return s;
    }
    if (add_stats) {
        c->st.reads += n;
        c->st.windows += n * (uint64_t)(L - c->k + 1);
    }
    return KC_OK;
}

kc_status kc_count_chunk_device(kc_ctx* c, const void* d_chunk, int64_t size, int64_t L) {
    if (!c || (!d_chunk && size > 0) || size < 0) return KC_ERR_ARG;
    kc_status s = check_line(c, L);
    if (s) return s;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if ((s = chunk_acc_flush(c))) return s;
    if ((s = chunk_device(c, (const uint8_t*)d_chunk, size, L))) return s;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's buffer was read by the encoder
    return KC_OK;
}

static kc_status copy_stream_init(kc_ctx* c) {
    if (c->copy_stream) return KC_OK;
    HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (auto& e : c->file_ev) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& e : c->stage_free) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return KC_OK;
}

// One staged upload + encode of host bytes (whole reads of length L): through
// the pinned ring (pageable source) or straight from a pinned buffer, into one
// of two staging buffers on the copy stream; the encode waits for that upload
// on the ctx stream, so the next upload overlaps this encode.
static kc_status chunk_upload_count(kc_ctx* c, const char* src, size_t bytes, int64_t L, bool pinned_src,
                                    hipEvent_t src_done, bool add_stats) {
    kc_status s;
    const int slot = c->chunk_slot;
    c->chunk_slot ^= 1;
    DevBuf& st = c->file_stage[slot];
    if (st.bytes < bytes + 64) {
        // growing: nothing may still read or write the old buffer
        HIPCHK(c, hipStreamSynchronize(c->copy_stream));
        if ((s = ensure(c, st, bytes + 64))) return s;
    }
    HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->stage_free[slot], 0));
    if (pinned_src) {
        HIPCHK(c, hipMemcpyAsync(st.p, src, bytes, hipMemcpyHostToDevice, c->copy_stream));
        if (src_done) HIPCHK(c, hipEventRecord(src_done, c->copy_stream));
    } else {
        HIPCHK(c, c->ring->upload(st.p, src, bytes, c->copy_stream, c->pool));
    }
    HIPCHK(c, hipEventRecord(c->file_ev[slot], c->copy_stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->file_ev[slot], 0));
    if ((s = chunk_device(c, (const uint8_t*)st.p, (int64_t)bytes, L, add_stats))) return s;
    HIPCHK(c, hipEventRecord(c->stage_free[slot], c->stream));
    return KC_OK;
}

static const size_t kAccBytes = (size_t)64 << 20;

// Uploads and counts the accumulated chunk reads (kc_count_chunk), if any.
static kc_status chunk_acc_flush(kc_ctx* c) {
    if (!c->count.acc_n) return KC_OK;
    const size_t bytes = c->count.acc_n;
    const int i = c->acc_i;
    c->count.acc_n = 0;  // first: counting may flush the pending batch, which comes back here
    c->acc_i ^= 1;
    c->acc_busy[i] = true;
    return chunk_upload_count(c, c->acc_buf[i], bytes, c->acc_L, true, c->acc_ev[i], false);
}

// Host chunk (the reference's readData output, KMerCounter.cpp:193-212: ~7.8
// MB at gpuMemoryLimit=1e8): its whole reads are copied into the pinned
// accumulation buffer (the call returns once the caller's bytes are copied);
// a full buffer (64 MB, about 8 such chunks) is uploaded and encoded while the
// next one fills, so per chunk the cost is the host copy and no device call.
// A chunk larger than half the buffer goes through the pinned ring directly.
kc_status kc_count_chunk(kc_ctx* c, const char* chunk, int64_t size, int64_t L) {
    if (!c || (!chunk && size > 0) || size < 0) return KC_ERR_ARG;
    kc_status s = check_line(c, L);
    if (s) return s;
    const uint64_t n = (uint64_t)(size / L);
    if (n == 0) return KC_OK;
    if (c->count.finished) return fail(c, KC_ERR_STATE, "kc_finish was called; kc_reset first");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if ((s = stage_init(c)) || (s = copy_stream_init(c))) return s;
    const size_t bytes = (size_t)(n * (uint64_t)L);
    const bool tr = kc::trace_on();
    double t0 = tr ? kc::now_s() : 0;
    if (tr) c->acc_t[3] += 1;
    if (c->count.acc_n && (c->acc_L != L || c->count.acc_n + bytes > kAccBytes))
        if ((s = chunk_acc_flush(c))) return s;
    if (tr) {
        const double t = kc::now_s();
        c->acc_t[2] += t - t0;
        t0 = t;
    }
    if (bytes > kAccBytes / 2) return chunk_upload_count(c, chunk, bytes, L, false, nullptr, true);
    const int i = c->acc_i;
    if (!c->acc_buf[i]) {
        HIPCHK(c, hipHostMalloc((void**)&c->acc_buf[i], kAccBytes, hipHostMallocDefault));
        HIPCHK(c, hipEventCreateWithFlags(&c->acc_ev[i], hipEventDisableTiming));
    }
    if (c->count.acc_n == 0) {
        if (c->acc_busy[i]) {  // its previous upload must be done before it is refilled
            HIPCHK(c, hipEventSynchronize(c->acc_ev[i]));
            c->acc_busy[i] = false;
        }
        c->acc_L = L;
    }
    if (tr) {
        const double t = kc::now_s();
        c->acc_t[1] += t - t0;
        t0 = t;
    }
    kc::par_memcpy(c->pool, c->acc_buf[i] + c->count.acc_n, chunk, bytes);
    if (tr) c->acc_t[0] += kc::now_s() - t0;
    c->count.acc_n += bytes;
    c->st.reads += n;
    c->st.windows += n * (uint64_t)(L - c->k + 1);
    return KC_OK;
}

static kc_status fastq_device(kc_ctx* c, const void* d_fastq, uint64_t n, int64_t L, uint64_t* n_reads,
                              bool count) {
    if (!c || (!d_fastq && n > 0)) return KC_ERR_ARG;
    if (n_reads) *n_reads = 0;
    if (n == 0) return KC_OK;
    if (count && c->count.finished) return fail(c, KC_ERR_STATE, "kc_finish was called; kc_reset first");
    if (L == 0) L = c->cfg.line_length;
    kc_status s = check_line(c, L);
    if (s) return s;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (count && (s = chunk_acc_flush(c))) return s;
    return ingest_fastq(c, (const uint8_t*)d_fastq, n, L, (c->cfg.flags & KC_FLAG_VARLEN) != 0, count, n_reads);
}

// Host FASTQ block: uploaded through the pinned ring (pageable) or directly
// (pinned), then decoded on the GPU (ingest_fastq, which waits for the
// checks: a malformed block is reported by this call).
static kc_status fastq_host(kc_ctx* c, const char* fastq, uint64_t n, int64_t L, uint64_t* n_reads, bool count) {
    if (!c || (!fastq && n > 0)) return KC_ERR_ARG;
    if (n_reads) *n_reads = 0;
    if (n == 0) return KC_OK;
    kc_status s;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if ((s = stage_init(c))) return s;
    if ((s = ensure(c, c->in_stage, (size_t)n + 64))) return s;
    HIPCHK(c, c->ring->upload(c->in_stage.p, fastq, n, c->stream, c->pool));
    return fastq_device(c, c->in_stage.p, n, L, n_reads, count);
}

kc_status kc_count_fastq_device(kc_ctx* c, const void* d_fastq, uint64_t n, int64_t L, uint64_t* n_reads) {
    return fastq_device(c, d_fastq, n, L, n_reads, true);
}

kc_status kc_count_fastq(kc_ctx* c, const char* fastq, uint64_t n, int64_t L, uint64_t* n_reads) {
    return fastq_host(c, fastq, n, L, n_reads, true);
}

kc_status kc_check_fastq(kc_ctx* c, const char* fastq, uint64_t n, int64_t L, uint64_t* n_reads) {
    return fastq_host(c, fastq, n, L, n_reads, false);
}

// ---- file input (InputFileHandler / FASTQFileReader + the Start loop) ----

static const size_t kFileBlock = (size_t)256 << 20;

// Block size of the file reader; KC_FILE_BLOCK (bytes) is a path selector for
// tests (many blocks from small files: cut search, carries; same counts).
static size_t file_block_bytes() {
    if (const char* e = test_hook("KC_FILE_BLOCK")) {
        const long long v = atoll(e);
        if (v >= 4096) return (size_t)v;
    }
    return kFileBlock;
}

// Uploads a block of the file reader (pinned) into staging buffer `slot` on
// the ctx's copy stream; the decode waits for it through file_ev[slot].
static kc_status file_upload(kc_ctx* c, int slot, const char* p, size_t n) {
    kc_status s;
    if ((s = copy_stream_init(c))) return s;
    if (c->file_stage[slot].bytes < n + 64) {
        HIPCHK(c, hipStreamSynchronize(c->copy_stream));
        if ((s = ensure(c, c->file_stage[slot], n + 64))) return s;
    }
    HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->stage_free[slot], 0));  // a chunk encode may still read it
    HIPCHK(c, hipMemcpyAsync(c->file_stage[slot].p, p, n, hipMemcpyHostToDevice, c->copy_stream));
    HIPCHK(c, hipEventRecord(c->file_ev[slot], c->copy_stream));
    return KC_OK;
}

// The GPU decode of an uploaded block (waits for its checks, hence for the
// upload: the reader may refill the host block when this returns). Kernels
// queued by the decode may still read the staging buffer (an encode of reads
// appended to the pending batch is not waited for), so the next upload into
// this slot waits for stage_free[slot], recorded after them.
static kc_status file_decode(kc_ctx* c, int slot, size_t n, int64_t L, bool count, uint64_t* got) {
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->file_ev[slot], 0));
    kc_status s = fastq_device(c, c->file_stage[slot].p, n, L, got, count);
    HIPCHK(c, hipEventRecord(c->stage_free[slot], c->stream));
    return s;
}

// Streams the file's blocks to the contexts (each block to whichever context
// is free: counting is order-independent). On the first failing block every
// context stops; *failed names the context that reported it.
static kc_status file_blocks(kc_ctx* const* ctxs, uint32_t n_ctx, const char* path, int64_t L, bool count,
                             uint64_t* reads, kc_ctx** failed) {
    // the reader's pinned buffers live in ctxs[0] (2 n_ctx + 2 of them: two per
    // context in flight, one filling, one holding the carried tail)
    kc_ctx* c0 = ctxs[0];
    const size_t block = file_block_bytes();
    const size_t want = block + kc::FastqFileReader::carry_bytes();
    if (c0->file_buf_bytes != want) {
        for (char* b : c0->file_bufs) (void)hipHostFree(b);
        c0->file_bufs.clear();
        c0->file_buf_bytes = want;
    }
    HIPCHK(c0, hipSetDevice(c0->cfg.device));
    while (c0->file_bufs.size() < 2 * (size_t)n_ctx + 2) {
        char* b = nullptr;
        HIPCHK(c0, hipHostMalloc((void**)&b, want, 0));
        c0->file_bufs.push_back(b);
    }
    std::vector<char*> bufs(c0->file_bufs.begin(), c0->file_bufs.begin() + 2 * n_ctx + 2);
    kc::FastqFileReader rd(block, bufs, 8);
    std::string err;
    *failed = ctxs[0];
    if (!rd.open(path, &err)) return fail(ctxs[0], KC_ERR_IO, "%s", err.c_str());
    std::atomic<bool> stop(false);
    std::vector<kc_status> st(n_ctx, KC_OK);
    std::vector<uint64_t> nr(n_ctx, 0);
    // per context: block i + 1 is uploaded (copy stream) while block i is
    // decoded (ctx stream)
    auto work = [&](uint32_t g) {
        kc_ctx* c = ctxs[g];
        if (hipSetDevice(c->cfg.device) != hipSuccess) {
            st[g] = fail(c, KC_ERR_HIP, "hipSetDevice(%d)", c->cfg.device);
            stop = true;
            return;
        }
        kc::FastqFileReader::Block cur, nxt;
        bool have = !stop && rd.next(&cur);
        int slot = 0;
        kc_status s = have ? file_upload(c, slot, cur.p, cur.n) : KC_OK;
        while (have && !s) {
            const bool have_nxt = !stop && rd.next(&nxt);
            if (have_nxt && (s = file_upload(c, slot ^ 1, nxt.p, nxt.n))) {
                rd.release(nxt);
                break;
            }
            uint64_t got = 0;
            const double t0 = kc::trace_on() ? kc::now_s() : 0;
            s = file_decode(c, slot, cur.n, L, count, &got);
            if (kc::trace_on()) kc::trace("ctx %u block %llu: %zu bytes, decode (+ upload wait) %.3f ms", g,
                                          (unsigned long long)cur.index, cur.n, (kc::now_s() - t0) * 1e3);
            rd.release(cur);
            nr[g] += got;
            if (s) {
                if (have_nxt) {
                    (void)hipStreamSynchronize(c->copy_stream);
                    rd.release(nxt);
                }
                break;
            }
            cur = nxt;
            have = have_nxt;
            slot ^= 1;
        }
        if (s) {
            st[g] = s;
            stop = true;
        }
    };
    if (n_ctx == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (uint32_t g = 0; g < n_ctx; g++) th.emplace_back(work, g);
        for (auto& t : th) t.join();
    }
    for (uint32_t g = 0; g < n_ctx; g++)
        if (st[g]) {
            *failed = ctxs[g];
            return st[g];
        }
    err = rd.error();
    if (!err.empty()) return fail(ctxs[0], KC_ERR_IO, "%s: %s", path, err.c_str());
    for (uint32_t g = 0; g < n_ctx; g++) *reads += nr[g];
    return KC_OK;
}

// inputMode=exact: the reference's chunks (ExactChunker, GetChunkSize with
// the ctx's gpuMemoryLimit) through kc_count_chunk.
static kc_status file_exact(kc_ctx* c, const char* path, int64_t L, uint64_t* reads) {
    const int64_t limit = c->cfg.gpu_memory_limit ? (int64_t)c->cfg.gpu_memory_limit : 100000000;
    const int64_t cs = kc::reference_chunk_size(L, c->k, limit);
    kc::ExactChunker ch(path, L);
    std::vector<char> buf;
    while (!ch.done()) {
        const int64_t n = ch.next(cs, buf);
        if (n > 0 && n >= L) {  // KMerCounter.cpp:130
            kc_status s = kc_count_chunk(c, buf.data(), n, L);
            if (s) return s;
            *reads += (uint64_t)(n / L);
        }
    }
    return KC_OK;
}

extern "C" kc_status kc_count_file(kc_ctx* const* ctxs, uint32_t n_ctx, const char* path, int64_t L, uint32_t mode,
                                   uint64_t* n_reads) {
    if (!ctxs || n_ctx == 0 || !path || mode > KC_INPUT_EXACT) return KC_ERR_ARG;
    for (uint32_t g = 0; g < n_ctx; g++)
        if (!ctxs[g] || ctxs[g]->k != ctxs[0]->k) return KC_ERR_ARG;
    kc_ctx* c0 = ctxs[0];
    const bool var = (c0->cfg.flags & KC_FLAG_VARLEN) != 0;
    if (n_reads) *n_reads = 0;
    if (L == 0) L = var ? c0->cfg.line_length : kc::file_line2_length(path);
    // reads shorter than k have no windows (the reference's CLI skips such files)
    if (L < c0->k) return KC_OK;
    kc_status s = check_line(c0, L);
    if (s) return s;
    for (uint32_t g = 0; g < n_ctx; g++) {  // chunks accumulated by kc_count_chunk are counted first
        HIPCHK(ctxs[g], hipSetDevice(ctxs[g]->cfg.device));
        if ((s = chunk_acc_flush(ctxs[g]))) return s;
    }
    uint64_t reads = 0;
    kc_ctx* failed = nullptr;
    if (mode == KC_INPUT_EXACT) {
        if (var) return fail(c0, KC_ERR_ARG, "variable-length reads have no reference chunk form");
        s = file_exact(c0, path, L, &reads);
    } else if (mode == KC_INPUT_FASTQ || var) {
        s = file_blocks(ctxs, n_ctx, path, L, true, &reads, &failed);
    } else {
        // auto: GPU decode; a malformed block sends the whole file to the
        // reference chunker. The file is read once when its reads fit every
        // context's checkpoint room (rolled back on a malformed block), else
        // it is validated first.
        struct stat sb;
        if (stat(path, &sb) != 0) return fail(c0, KC_ERR_IO, "cannot stat %s: %s", path, strerror(errno));
        const uint64_t est = (uint64_t)sb.st_size / (uint64_t)(2 * L + 6) + 1;  // records are >= 2L + 6 bytes
        bool once = true;
        for (uint32_t g = 0; g < n_ctx; g++) {
            kc_ctx* c = ctxs[g];
            c->count.ckpt = true;
            const uint64_t room = pend_room(c, L);
            c->count.ckpt = false;
            if ((c->count.pend_reads && (c->count.pend_L != L || c->count.pend_var)) || (c->count.pend_L == L ? c->count.pend_reads : 0) + est > room)
                once = false;
        }
        bool exact = false;
        if (once) {
            for (uint32_t g = 0; g < n_ctx; g++)
                if ((s = kc_checkpoint(ctxs[g]))) return s;
            s = file_blocks(ctxs, n_ctx, path, L, true, &reads, &failed);
            if (s == KC_ERR_FORMAT) {
                for (uint32_t g = 0; g < n_ctx; g++) {
                    kc_status r = kc_rollback(ctxs[g]);
                    if (r) return r;
                }
                exact = true;
                reads = 0;
            } else {
                for (uint32_t g = 0; g < n_ctx; g++) kc_commit(ctxs[g]);
            }
        } else {
            uint64_t dummy = 0;
            s = file_blocks(ctxs, n_ctx, path, L, false, &dummy, &failed);
            if (s == KC_ERR_FORMAT) {
                exact = true;
            } else if (!s) {
                s = file_blocks(ctxs, n_ctx, path, L, true, &reads, &failed);
            }
        }
        if (exact) s = file_exact(c0, path, L, &reads);
    }
    if (s) {
        if (failed && failed != c0) c0->err = failed->err;  // the caller reads ctxs[0]'s message
        return s;
    }
    if (n_reads) *n_reads = reads;
    return KC_OK;
}

kc_status kc_checkpoint(kc_ctx* c) {
    if (!c) return KC_ERR_ARG;
    if (c->count.finished) return fail(c, KC_ERR_STATE, "kc_finish was called; kc_reset first");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    kc_status s = chunk_acc_flush(c);  // accumulated chunks are counted before the checkpoint
    if (s) return s;
    s = sync_stats(c);
    if (s) return s;
    c->count.ckpt = true;
    c->ckpt_reads = c->count.pend_reads;
    c->ckpt_flushes = c->flushes;
    c->ckpt_st_reads = c->st.reads;
    c->ckpt_st_windows = c->st.windows;
    memcpy(c->ckpt_stats, c->stats_h, sizeof(c->ckpt_stats));
    return KC_OK;
}

kc_status kc_rollback(kc_ctx* c) {
    if (!c) return KC_ERR_ARG;
    if (!c->count.ckpt) return fail(c, KC_ERR_STATE, "no checkpoint");
    c->count.ckpt = false;
    if (c->flushes != c->ckpt_flushes || c->count.finished)
        return fail(c, KC_ERR_STATE, "reads were counted since the checkpoint: it cannot be rolled back");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    c->count.pend_reads = c->ckpt_reads;
    if (c->count.pend_reads == 0) c->count.pend_sparse = false;  // (rows kept keep their lengths)
    c->count.acc_n = 0;  // chunks accumulated since (kc_checkpoint flushed the accumulator) are forgotten too
    c->st.reads = c->ckpt_st_reads;
    c->st.windows = c->ckpt_st_windows;
    HIPCHK(c, hipMemcpyAsync(c->stats, c->ckpt_stats, sizeof(c->ckpt_stats), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(c->stats_h, c->ckpt_stats, sizeof(c->ckpt_stats));
    return KC_OK;
}

kc_status kc_commit(kc_ctx* c) {
    if (!c) return KC_ERR_ARG;
    c->count.ckpt = false;
    return KC_OK;
}

kc_status kc_copy_records(kc_ctx* c, void* dst, uint64_t dst_bytes) {
    if (!c || !dst) return KC_ERR_ARG;
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    if (!c->runs.empty()) return fail(c, KC_ERR_STATE, "spill runs exist: use kc_write_output");
    uint64_t bytes = c->count.n_records * c->rs;
    if (dst_bytes < bytes) return fail(c, KC_ERR_ARG, "destination holds %llu bytes, need %llu",
                                       (unsigned long long)dst_bytes, (unsigned long long)bytes);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (bytes) {
        HIPCHK(c, hipMemcpyAsync(dst, c->fin_packed.p, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return KC_OK;
}

kc_status kc_device_records(kc_ctx* c, const void** d_records, uint64_t* n_bytes) {
    if (!c || !d_records || !n_bytes) return KC_ERR_ARG;
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    *d_records = c->fin_packed.p;
    *n_bytes = c->count.n_records * c->rs;
    return KC_OK;
}

// The finished table run (SortedKMerFile bytes) to host memory through the
// pinned ring, the pieces copied out by the pool while the next DMA runs.
static kc_status table_run_to_host(kc_ctx* c, std::vector<uint8_t>* mem) {
    const uint64_t bytes = c->count.n_records * c->rs;
    mem->resize(bytes);
    if (!bytes) return KC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    kc_status s = stage_init(c);
    if (s) return s;
    uint8_t* dst = mem->data();
    HIPCHK(c, c->ring->download(c->fin_packed.p, bytes, c->stream, [&](const char* p, size_t n, size_t off) {
        kc::par_memcpy(c->pool, dst + off, p, n);
        return true;
    }));
    return KC_OK;
}

// The finished table run into a file at byte `at` (`whole`: the file is
// exactly the run, as after truncating it — the reference appends,
// KMerFileMerger.cpp:129): device -> pinned slot DMAs overlap the writes of
// the previous slot. An existing file is not truncated first but overwritten
// in place and cut to size at the end (truncating a cached file frees its
// pages, ~60 ms per GB, and the writes then allocate them again); the range
// is allocated up front (fallocate), the writes go out in 8 MiB pieces.
static kc_status table_run_to_file(kc_ctx* c, const char* path, uint64_t at = 0, bool whole = true) {
    const uint64_t bytes = c->count.n_records * c->rs;
    const double t0 = kc::trace_on() ? kc::now_s() : 0;
    int fd = open(path, O_CREAT | O_WRONLY, 0644);
    if (fd < 0) return fail(c, KC_ERR_IO, "cannot open output file %s: %s", path, strerror(errno));
    // the range is reserved up front: a full filesystem fails here, by name,
    // before any byte moves (filesystems without fallocate just write)
    if (bytes && fallocate(fd, 0, (off_t)at, (off_t)bytes) != 0 && errno != EOPNOTSUPP && errno != ENOSYS) {
        const int e = errno;
        close(fd);
        return fail(c, KC_ERR_IO, "cannot reserve %llu bytes at %llu in %s: %s", (unsigned long long)bytes,
                    (unsigned long long)at, path, strerror(e));
    }
    if (kc::trace_on()) kc::trace("output open + fallocate %.3f ms", (kc::now_s() - t0) * 1e3);
    kc_status s = KC_OK;
    if (bytes) {
        HIPCHK(c, hipSetDevice(c->cfg.device));
        if ((s = stage_init(c))) {
            close(fd);
            return s;
        }
        int werr = 0;
        uint64_t wat = 0;
        hipError_t e = c->ring->download(c->fin_packed.p, bytes, c->stream, [&](const char* p, size_t n, size_t off) {
            size_t done = 0;
            while (done < n) {
                const size_t piece = std::min((size_t)8 << 20, n - done);
                ssize_t w = pwrite(fd, p + done, piece, (off_t)(at + off + done));
                if (w < 0 && errno == EINTR) continue;
                if (w <= 0) {
                    werr = w < 0 ? errno : ENOSPC;  // a 0-byte write: no room
                    wat = at + off + done;
                    return false;
                }
                done += (size_t)w;
            }
            return true;
        });
        if (e == hipErrorUnknown)
            s = fail(c, KC_ERR_IO, "write to %s failed at byte %llu of %llu: %s", path, (unsigned long long)wat,
                     (unsigned long long)(at + bytes), strerror(werr));
        else if (e != hipSuccess) s = fail(c, KC_ERR_HIP, "output copy: %s", hipGetErrorString(e));
    }
    if (!s && whole && ftruncate(fd, (off_t)(at + bytes)) != 0)
        s = fail(c, KC_ERR_IO, "cannot size %s: %s", path, strerror(errno));
    if (close(fd) != 0 && !s) s = fail(c, KC_ERR_IO, "cannot close %s: %s", path, strerror(errno));
    if (kc::trace_on()) kc::trace("output %llu bytes in %.3f ms", (unsigned long long)bytes, (kc::now_s() - t0) * 1e3);
    return s;
}

kc_status kc_write_output(kc_ctx* c, const char* path, uint32_t fan_in, uint32_t threads) {
    if (!c || !path) return KC_ERR_ARG;
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    if (c->runs.empty()) return table_run_to_file(c, path);
    std::vector<uint8_t> table_run;
    kc_status s = table_run_to_host(c, &table_run);
    if (s) return s;
    std::vector<RunSource> src;
    RunSource t;
    t.mem = table_run.data();
    t.bytes = table_run.size();
    src.push_back(t);
    for (auto& r : c->runs) {
        RunSource x;
        if (!r.path.empty())
            x.path = r.path;
        else {
            x.mem = r.mem.data();
            x.bytes = r.mem.size();
        }
        src.push_back(x);
    }
    std::string err;
    std::string tmp_prefix = std::string(path) + ".kctmp";
    if (!merge_tree(src, path, c->W, fan_in, threads, tmp_prefix, &err))
        return fail(c, KC_ERR_IO, "%s", err.c_str());
    return KC_OK;
}

kc_status kc_write_output_at(kc_ctx* c, const char* path, uint64_t offset) {
    if (!c || !path) return KC_ERR_ARG;
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    if (!c->runs.empty()) return fail(c, KC_ERR_STATE, "spill runs exist: use kc_write_output");
    return table_run_to_file(c, path, offset, false);
}

kc_status kc_write_runs(kc_ctx* c, const char* prefix, uint32_t* n_runs) {
    if (!c || !prefix) return KC_ERR_ARG;
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    std::vector<uint8_t> table_run;
    kc_status s = table_run_to_host(c, &table_run);
    if (s) return s;
    uint32_t count = 0;
    auto write_one = [&](const uint8_t* p, size_t bytes, const std::string& from) -> kc_status {
        std::string name = std::string(prefix) + "." + std::to_string(count);
        if (!from.empty()) {
            // copy the temp file
            FILE* in = fopen(from.c_str(), "rb");
            FILE* out = fopen(name.c_str(), "wb");
            if (!in || !out) {
                if (in) fclose(in);
                if (out) fclose(out);
                return fail(c, KC_ERR_IO, "cannot copy run %s to %s: %s", from.c_str(), name.c_str(), strerror(errno));
            }
            std::vector<char> buf(1 << 20);
            size_t got;
            while ((got = fread(buf.data(), 1, buf.size(), in)) > 0) fwrite(buf.data(), 1, got, out);
            fclose(in);
            fclose(out);
        } else {
            FILE* out = fopen(name.c_str(), "wb");
            if (!out) return fail(c, KC_ERR_IO, "cannot write run %s: %s", name.c_str(), strerror(errno));
            size_t w = bytes ? fwrite(p, 1, bytes, out) : 0;
            const int we = errno;
            const int ce = fclose(out) != 0 ? errno : 0;
            if (w != bytes || ce) return fail(c, KC_ERR_IO, "short write %s: %s", name.c_str(), strerror(w != bytes ? we : ce));
        }
        count++;
        return KC_OK;
    };
    if ((s = write_one(table_run.data(), table_run.size(), ""))) return s;
    for (auto& r : c->runs)
        if ((s = write_one(r.mem.data(), r.mem.size(), r.path))) return s;
    if (n_runs) *n_runs = count;
    return KC_OK;
}

kc_status kc_get_stats(const kc_ctx* c, kc_stats* out) {
    if (!c || !out) return KC_ERR_ARG;
    *out = c->st;
    out->insert_launches = c->count.insert_launches;
    out->insert_ms = c->count.insert_ms;
    for (int i = 0; i < 5; i++) out->part_ms[i] = c->count.part_ms[i];
    out->presplit_ms = c->count.presplit_ms;
    out->presplit_batches = c->count.presplit_batches;
    out->sorted_run_batches = c->count.sorted_run_batches;
    out->key_passes = c->count.key_passes;
    out->batches = c->count.batches_cut + c->count.batches;
    out->keys = c->count.part_keys;
    out->p5_launches = c->count.p5_launches;
    out->table_capacity = c->cap;
    out->valid_kmers = c->stats_h[ST_VALID];
    out->spill_runs = c->count.runs_cut + c->runs.size();
    out->engines_used = c->count.engines_used;
    out->dedup_ms = c->count.dedup_ms;
    out->dedup_records = c->stats_h[ST_DEDUP];
    out->finish_group_ms = c->count.finish_group_ms;
    return KC_OK;
}

kc_status kc_merge_files(const char* const* inputs, uint32_t n_inputs, const char* output, int64_t kmer_length,
                         uint32_t fan_in, uint32_t threads) {
    if (!output || kmer_length < 1 || kmer_length > KC_MAX_K || (n_inputs && !inputs)) return KC_ERR_ARG;
    int W = (int)((kmer_length + 31) / 32);
    std::vector<RunSource> src;
    for (uint32_t i = 0; i < n_inputs; i++) {
        RunSource r;
        r.path = inputs[i];
        src.push_back(r);
    }
    std::string err;
    if (!merge_tree(src, output, W, fan_in, threads, std::string(output) + ".kctmp", &err)) return KC_ERR_IO;
    return KC_OK;
}

struct kc_merge_part {
    kc::MergedPart part;
};

kc_status kc_merge_part_create(const char* const* inputs, uint32_t n_inputs, int64_t kmer_length, uint32_t part,
                               uint32_t parts, uint32_t threads, kc_merge_part** out, uint64_t* n_bytes) {
    if (!out || kmer_length < 1 || kmer_length > KC_MAX_K || (n_inputs && !inputs) || parts < 1 || part >= parts)
        return KC_ERR_ARG;
    *out = nullptr;
    const int W = (int)((kmer_length + 31) / 32);
    std::vector<RunSource> src;
    for (uint32_t i = 0; i < n_inputs; i++) {
        if (!inputs[i]) return KC_ERR_ARG;
        RunSource r;
        r.path = inputs[i];
        src.push_back(r);
    }
    std::unique_ptr<kc_merge_part> p(new (std::nothrow) kc_merge_part());
    if (!p) return KC_ERR_NOMEM;
    int e = 0;
    try {
        if (!kc::merge_runs_part(src, W, part, parts, threads ? threads : 1, &p->part, &e)) return KC_ERR_IO;
    } catch (const std::bad_alloc&) {
        return KC_ERR_NOMEM;
    }
    if (n_bytes) *n_bytes = p->part.bytes;
    *out = p.release();
    return KC_OK;
}

kc_status kc_merge_part_write(kc_merge_part* p, const char* output, uint64_t offset, uint64_t file_bytes) {
    if (!p || !output) return KC_ERR_ARG;
    if (file_bytes && offset + p->part.bytes > file_bytes) return KC_ERR_ARG;
    return kc::write_part_at(p->part, output, offset, file_bytes) ? KC_OK : KC_ERR_IO;
}

void kc_merge_part_destroy(kc_merge_part* p) { delete p; }

uint64_t kc_synth_fastq_bytes(const kc_synth_spec* sp) {
    if (!sp) return 0;
    return synth_bytes(sp->first_read, sp->n_reads, sp->read_length, (int)sp->layout);
}

static SynthArgs synth_args(const kc_synth_spec* sp) {
    SynthArgs a;
    a.first = sp->first_read;
    a.n = sp->n_reads;
    a.seed = sp->seed;
    a.genome = sp->genome_length;
    a.L = sp->read_length;
    a.Lmin = sp->min_read_length;
    a.layout = (int)sp->layout;
    double thr = sp->n_rate * 9007199254740992.0;
    a.n_threshold = sp->n_rate <= 0 ? 0 : (thr >= 9007199254740992.0 ? (1ull << 53) : (uint64_t)thr);
    return a;
}

static bool synth_ok(const kc_synth_spec* sp) {
    return sp && sp->read_length > 0 && (sp->genome_length == 0 || sp->genome_length >= (uint64_t)sp->read_length) &&
           sp->min_read_length >= 0 && sp->min_read_length <= sp->read_length && sp->layout <= 1 &&
           (sp->layout == 0 || sp->min_read_length == 0 || sp->min_read_length == sp->read_length);
}

kc_status kc_synth_fastq_host(const kc_synth_spec* sp, char* dst, uint64_t dst_bytes) {
    if (!synth_ok(sp) || !dst) return KC_ERR_ARG;
    if (dst_bytes < kc_synth_fastq_bytes(sp)) return KC_ERR_ARG;
    synth_host(synth_args(sp), dst);
    return KC_OK;
}

kc_status kc_synth_fastq_device(kc_ctx* c, const kc_synth_spec* sp, void** d_out, uint64_t* n_bytes) {
    if (!c || !synth_ok(sp) || !d_out) return KC_ERR_ARG;
    uint64_t bytes = kc_synth_fastq_bytes(sp);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    void* p = nullptr;
    HIPCHK(c, hipMalloc(&p, bytes + 64));
    HIPCHK(c, launch_synth(synth_args(sp), (char*)p, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *d_out = p;
    if (n_bytes) *n_bytes = bytes;
    return KC_OK;
}

kc_status kc_synth_free(kc_ctx* c, void* d_buf) {
    if (!c) return KC_ERR_ARG;
    if (d_buf) HIPCHK(c, hipFree(d_buf));
    return KC_OK;
}

kc_status kc_owner_counts(kc_ctx* c, uint32_t world, uint64_t* counts) {
    if (!c || world == 0 || !counts) return KC_ERR_ARG;
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    if (!c->runs.empty()) return fail(c, KC_ERR_STATE, "spill runs exist: the key-space exchange needs one run");
    kc_status s;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if ((s = ensure(c, c->part_starts, ((size_t)world + 1) * 8))) return s;
    HIPCHK(c, launch_owner_bounds(c->fin_packed.p, c->rs, c->count.n_records, world, c->part_starts.as<uint64_t>(), c->stream));
    std::vector<uint64_t> b(world + 1);
    HIPCHK(c, hipMemcpyAsync(b.data(), c->part_starts.p, (world + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t o = 0; o < world; o++) counts[o] = b[o + 1] - b[o];
    return KC_OK;
}


// ---- queries on the finished run ------------------------------------------

// The state rules the queries share with kc_copy_records.
static kc_status query_state(kc_ctx* c) {
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    if (!c->runs.empty()) return fail(c, KC_ERR_STATE, "spill runs exist: write the output and use the file form");
    return KC_OK;
}

kc_status kc_count_histogram(kc_ctx* c, uint64_t* bins, uint32_t n_bins) {
    if (!c || !bins) return KC_ERR_ARG;
    if (n_bins < 2 || n_bins > 65536) return fail(c, KC_ERR_ARG, "n_bins %u outside [2, 65536]", n_bins);
    kc_status s;
    if ((s = query_state(c))) return s;
    memset(bins, 0, (size_t)n_bins * 8);
    if (c->count.n_records == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if ((s = ensure(c, c->q_bins, (size_t)n_bins * 8 + 8))) return s;
    HIPCHK(c, hipMemsetAsync(c->q_bins.p, 0, (size_t)n_bins * 8, c->stream));
    HIPCHK(c, launch_count_histo(c->fin_packed.p, c->W, c->count.n_records, n_bins, c->q_bins.as<uint64_t>(), c->stream));
    HIPCHK(c, hipMemcpyAsync(bins, c->q_bins.p, (size_t)n_bins * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KC_OK;
}

kc_status kc_filter_records(kc_ctx* c, uint32_t min_count, uint32_t max_count, uint64_t* n_kept) {
    if (!c) return KC_ERR_ARG;
    if (min_count > max_count) return fail(c, KC_ERR_ARG, "min_count %u > max_count %u", min_count, max_count);
    kc_status s;
    if ((s = query_state(c))) return s;
    const uint64_t n = c->count.n_records;
    if (n_kept) *n_kept = n;
    if (n == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // tile counts, their exclusive scan, the scan's scratch, the total
    const uint64_t ntiles = (n + filter_tile() - 1) / filter_tile();
    if ((s = ensure(c, c->q_tiles, (2 * ntiles + scan_tmp_elems(ntiles) + 1) * 8))) return s;
    uint64_t* cnt = c->q_tiles.as<uint64_t>();
    uint64_t* base = cnt + ntiles;
    uint64_t* total = base + ntiles;
    uint64_t* tmp = total + 1;
    HIPCHK(c, launch_filter_count(c->fin_packed.p, c->W, n, min_count, max_count, cnt, c->stream));
    HIPCHK(c, launch_scan_u64(cnt, base, ntiles, tmp, c->stream));
    HIPCHK(c, launch_sum_last(base, cnt, ntiles, total, c->stream));
    uint64_t kept = 0;
    HIPCHK(c, hipMemcpyAsync(&kept, total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (kept > n) return fail(c, KC_ERR_INTERNAL, "filter kept %llu of %llu records", (unsigned long long)kept,
                              (unsigned long long)n);
    if (kept != 0 && kept != n) {
        // out of place: the kept records into a pooled buffer that becomes the
        // run; the old buffer joins the pool, as kc_finish and the merges do
        DevBuf dst;
        if ((s = ensure_pooled(c, dst, (size_t)kept * c->rs + 16))) return s;
        hipError_t e = launch_filter_scatter(c->fin_packed.p, c->W, n, min_count, max_count, base, dst.p, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            c->run_pool.push_back(std::move(dst));
            return fail(c, KC_ERR_HIP, "filter scatter: %s", hipGetErrorString(e));
        }
        c->run_pool.push_back(std::move(c->fin_packed));
        c->fin_packed = std::move(dst);
    }
    c->count.n_records = kept;
    c->st.output_records = kept;
    if (n_kept) *n_kept = kept;
    return KC_OK;
}

kc_status kc_lookup_device(kc_ctx* c, const void* d_keys, uint64_t n_keys, void* d_counts, void* d_found,
                           uint64_t* n_found) {
    if (!c || (n_keys && (!d_keys || !d_counts))) return KC_ERR_ARG;
    kc_status s;
    if ((s = query_state(c))) return s;
    if (n_found) *n_found = 0;
    if (n_keys == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if ((s = ensure(c, c->q_bins, 8))) return s;
    HIPCHK(c, hipMemsetAsync(c->q_bins.p, 0, 8, c->stream));
    HIPCHK(c, launch_lookup(c->fin_packed.p, c->W, c->count.n_records, (const uint64_t*)d_keys, n_keys, (uint32_t*)d_counts,
                            (uint8_t*)d_found, c->q_bins.as<uint64_t>(), c->stream));
    uint64_t nf = 0;
    HIPCHK(c, hipMemcpyAsync(&nf, c->q_bins.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_found) *n_found = nf;
    return KC_OK;
}

kc_status kc_lookup(kc_ctx* c, const uint64_t* keys, uint64_t n_keys, uint32_t* counts, uint8_t* found,
                    uint64_t* n_found) {
    if (!c || (n_keys && (!keys || !counts))) return KC_ERR_ARG;
    kc_status s;
    if ((s = query_state(c))) return s;
    if (n_found) *n_found = 0;
    if (n_keys == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const size_t kb = (size_t)n_keys * c->W * 8;
    if ((s = ensure(c, c->q_keys, kb)) || (s = ensure(c, c->q_counts, (size_t)n_keys * 4)) ||
        (s = ensure(c, c->q_found, (size_t)n_keys)))
        return s;
    HIPCHK(c, hipMemcpyAsync(c->q_keys.p, keys, kb, hipMemcpyHostToDevice, c->stream));
    if ((s = kc_lookup_device(c, c->q_keys.p, n_keys, c->q_counts.p, c->q_found.p, n_found))) return s;
    HIPCHK(c, hipMemcpyAsync(counts, c->q_counts.p, (size_t)n_keys * 4, hipMemcpyDeviceToHost, c->stream));
    if (found) HIPCHK(c, hipMemcpyAsync(found, c->q_found.p, (size_t)n_keys, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KC_OK;
}

kc_status kc_histogram_file(const char* path, int64_t kmer_length, uint64_t* bins, uint32_t n_bins) {
    if (!path || !bins || kmer_length < 1 || kmer_length > KC_MAX_K || n_bins < 2 || n_bins > 65536)
        return KC_ERR_ARG;
    return kc::histogram_file(path, (int)((kmer_length + 31) / 32), bins, n_bins) ? KC_OK : KC_ERR_IO;
}

kc_status kc_filter_file(const char* input, const char* output, int64_t kmer_length, uint32_t min_count,
                         uint32_t max_count, uint64_t* n_kept) {
    if (!input || !output || kmer_length < 1 || kmer_length > KC_MAX_K || min_count > max_count) return KC_ERR_ARG;
    return kc::filter_file(input, output, (int)((kmer_length + 31) / 32), min_count, max_count, n_kept) ? KC_OK
                                                                                                         : KC_ERR_IO;
}

kc_status kc_canonicalize_file(const char* input, const char* output, int64_t kmer_length, uint64_t* n_records) {
    if (!input || !output || kmer_length < 1 || kmer_length > KC_MAX_K) return KC_ERR_ARG;
    return kc::canonicalize_file(input, output, (int)kmer_length, n_records) ? KC_OK : KC_ERR_IO;
}

// ---- set operations between two finished runs ------------------------------

static bool setop_ok(uint32_t op, uint32_t mode) {
    if (op > KC_SET_COUNT_SUBTRACT || mode > KC_SETC_RIGHT) return false;
    return op <= KC_SET_INTERSECT || mode == KC_SETC_SUM;
}

// `dst` (a pooled buffer that holds the result) becomes the finished run of
// n records; the old run joins the pool, as after kc_filter_records.
static void install_run(kc_ctx* c, DevBuf& dst, uint64_t n) {
    if (dst.p) {
        if (c->fin_packed.p) c->run_pool.push_back(std::move(c->fin_packed));
        c->fin_packed = std::move(dst);
    }
    c->count.n_records = n;
    c->st.output_records = n;
}

kc_status kc_combine_records_device(kc_ctx* c, const void* d_packed, uint64_t n_records, uint32_t op,
                                    uint32_t count_mode, uint64_t* n_out) {
    if (!c || (n_records && !d_packed)) return KC_ERR_ARG;
    if (!setop_ok(op, count_mode)) return fail(c, KC_ERR_ARG, "set operation %u with count mode %u", op, count_mode);
    kc_status s;
    if ((s = query_state(c))) return s;
    const uint64_t na = c->count.n_records, nb = n_records;
    const size_t rs = (size_t)c->rs;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    DevBuf dst;
    uint64_t nout = 0;
    if (na == 0 || nb == 0) {
        // an empty operand: nothing to merge. The result is A, B or empty.
        if (nb == 0 && op != KC_SET_INTERSECT) {
            nout = na;
        } else if (na == 0 && op == KC_SET_UNION) {
            if ((s = ensure_pooled(c, dst, (size_t)nb * rs + 16))) return s;
            hipError_t e = hipMemcpyAsync(dst.p, d_packed, (size_t)nb * rs, hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) {
                c->run_pool.push_back(std::move(dst));
                return fail(c, KC_ERR_HIP, "combine copy: %s", hipGetErrorString(e));
            }
            nout = nb;
        }
        install_run(c, dst, nout);
        if (n_out) *n_out = nout;
        return KC_OK;
    }
    const uint64_t n = na + nb;
    const uint64_t ntiles = (n + (uint64_t)setop_tile(c->W) - 1) / (uint64_t)setop_tile(c->W);
    // the tile splits; tile counts, their exclusive scan, the total, the scan's scratch
    if ((s = ensure(c, c->fin_misc, merge_packed_split_elems(c->W, n) * 8)) ||
        (s = ensure(c, c->q_tiles, (2 * ntiles + scan_tmp_elems(ntiles) + 1) * 8)))
        return s;
    uint64_t* split = c->fin_misc.as<uint64_t>();
    uint64_t* cnt = c->q_tiles.as<uint64_t>();
    uint64_t* base = cnt + ntiles;
    uint64_t* total = base + ntiles;
    uint64_t* tmp = total + 1;
    HIPCHK(c, launch_setop_count(c->W, c->fin_packed.p, na, d_packed, nb, op, count_mode, split, cnt, c->stream));
    HIPCHK(c, launch_scan_u64(cnt, base, ntiles, tmp, c->stream));
    HIPCHK(c, launch_sum_last(base, cnt, ntiles, total, c->stream));
    HIPCHK(c, hipMemcpyAsync(&nout, total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nout > n) return fail(c, KC_ERR_INTERNAL, "combine kept %llu of %llu records", (unsigned long long)nout,
                              (unsigned long long)n);
    if (nout) {
        if ((s = ensure_pooled(c, dst, (size_t)nout * rs + 16))) return s;
        hipError_t e = launch_setop_emit(c->W, c->fin_packed.p, na, d_packed, nb, op, count_mode, split, base, dst.p,
                                         c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            c->run_pool.push_back(std::move(dst));
            return fail(c, KC_ERR_HIP, "combine emit: %s", hipGetErrorString(e));
        }
    }
    install_run(c, dst, nout);
    if (n_out) *n_out = nout;
    return KC_OK;
}

kc_status kc_combine_contexts(kc_ctx* a, kc_ctx* b, uint32_t op, uint32_t count_mode, uint64_t* n_out) {
    if (!a || !b) return KC_ERR_ARG;
    if (a == b) return fail(a, KC_ERR_ARG, "combine: both operands are the same context");
    if (a->k != b->k) return fail(a, KC_ERR_ARG, "combine: kmer_length %lld and %lld", (long long)a->k, (long long)b->k);
    if (!setop_ok(op, count_mode)) return fail(a, KC_ERR_ARG, "set operation %u with count mode %u", op, count_mode);
    kc_status s;
    if ((s = query_state(a))) return s;
    if (query_state(b)) return fail(a, KC_ERR_STATE, "combine: the second context: %s", b->err.c_str());
    const uint64_t nb = b->count.n_records;
    if (a->cfg.device == b->cfg.device || nb == 0)
        return kc_combine_records_device(a, nb ? b->fin_packed.p : nullptr, nb, op, count_mode, n_out);
    // b's run comes over to a's device, as kc_gather_contexts copies runs
    HIPCHK(a, hipSetDevice(a->cfg.device));
    DevBuf recv;
    HIPCHK(a, recv.alloc((size_t)nb * a->rs + 16));
    HIPCHK(a, hipMemcpyPeerAsync(recv.p, a->cfg.device, b->fin_packed.p, b->cfg.device, (size_t)nb * a->rs, a->stream));
    HIPCHK(a, hipStreamSynchronize(a->stream));
    return kc_combine_records_device(a, recv.p, nb, op, count_mode, n_out);
}

kc_status kc_combine_files(const char* a, const char* b, const char* output, int64_t kmer_length, uint32_t op,
                           uint32_t count_mode, uint64_t* n_out) {
    if (!a || !b || !output || kmer_length < 1 || kmer_length > KC_MAX_K || !setop_ok(op, count_mode))
        return KC_ERR_ARG;
    return kc::combine_files(a, b, output, (int)((kmer_length + 31) / 32), op, count_mode, n_out) ? KC_OK : KC_ERR_IO;
}

kc_status kc_copy_device(kc_ctx* c, void* d_dst, const void* d_src, uint64_t n) {
    if (!c || (n && (!d_dst || !d_src))) return KC_ERR_ARG;
    if (n == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipMemcpyAsync(d_dst, d_src, n, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KC_OK;
}

kc_status kc_copy_to_host(kc_ctx* c, void* dst, const void* d_src, uint64_t n) {
    if (!c || (n && (!dst || !d_src))) return KC_ERR_ARG;
    if (n == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipMemcpyAsync(dst, d_src, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KC_OK;
}

}  // extern "C"
