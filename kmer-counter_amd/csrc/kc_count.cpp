// kc_count.cpp — counting: the three engines (table, key-prefix "partition",
// super-k-mer) that turn reads into records, the choice between them
// (engine_for, the coverage sketch), and how many pre-encoded reads go to them
// per call (count_pending_fixed). Ingest (kc_ingest.cpp) feeds count_reads.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "kc_ctx.h"

static uint32_t probe_limit(const kc_ctx* c) {
    // a nearly full table: give up early and spill instead of walking long runs
    uint64_t used = c->stats_h[ST_CLAIMED];
    if (used * 10 >= c->cap * 9) return 8;
    return c->W == 1 ? 128 : 64;
}

// The launch arguments of reads [read0, read0 + nr) of a count call. pre0 >= 0:
// the reads are already encoded in part_codes / part_inval (/ var_rlen) from
// read index pre0 on; else kernel E writes them at the buffers' start.
CountLaunch make_launch(const kc_ctx* c, const uint8_t* base, const uint64_t* seq_off, uint64_t read0, uint64_t nr,
                        int64_t L, int64_t pre0) {
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

// No records, batches or runs yet: gates P5s direct and the key-range passes,
// whose run is the whole result (an empty global table is each site's own term)
static bool records_empty(const kc_ctx* c) {
    return c->count.rec_n == 0 && c->count.batches == 0 && !c->count.skm_used && c->runs.empty();
}

// v reads per batch or slice, made even when a read's code row is an odd
// number of words: every batch's masks then start 4-byte aligned, which F3's
// dword DMA needs
static uint64_t even_reads(int64_t L, uint64_t v) { return (groups_per_read((int)L) & 1) && v > 1 ? v & ~1ull : v; }

// Engine "table": every k-mer is inserted into the global HBM table with
// atomics. Counts n_reads reads (stride mode when seq_off == nullptr).
static kc_status count_reads_table(kc_ctx* c, const uint8_t* base, const uint64_t* seq_off, uint64_t n_reads,
                                   int64_t L) {
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
        if (nr * nw > free_slots && (s = flush_spill(c))) return s;
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

// The engine that counts reads of length L now: skm while it is chosen, not
// handed over (skm_hc) and has a geometry for (L, k); else key-prefix when one
// read's windows fit a P2 workgroup's LDS; else (very long reads,
// KC_FLAG_ENGINE_TABLE) the table engine. All feed the same finish.
Engine engine_for(const kc_ctx* c, int64_t L) {
    if (c->skm && !c->count.skm_hc && skm_geometry((int)L, (int)c->k).ok) return Engine::skm;
    if (c->part && part_geometry((int)L, (int)c->k, 1).lds_scatter <= kMaxLds) return Engine::prefix;
    return Engine::table;
}

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
static kc_status p5s_direct(kc_ctx* c, const uint64_t* keys, uint64_t kstride, const uint64_t* sub_starts, uint32_t nb,
                            uint64_t n, uint8_t* rf, size_t fl, bool* done, uint64_t* records, float* ms,
                            uint64_t pk_at = 0, uint64_t total = 0, bool last = true) {
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
    const uint64_t nw = (uint64_t)(L - c->k + 1);
    const uint64_t max_reads = c->key_cap / nw;
    if (max_reads == 0) return fail(c, KC_ERR_ARG, "gpu_memory_limit too small for one read's windows");
    kc_status s;
    uint64_t done = 0;
    KeyPasses kp;
    const bool p2_no_digs = test_hook("KC_P2_NO_DIGS") != nullptr;
    const bool p2_aos = !p2_no_digs && !test_hook("KC_P2_SOA");
    if (pre0 >= 0 && c->count.hc_hint && nw * n_reads > c->key_cap && records_empty(c) &&
        c->stats_h[ST_CLAIMED] == 0 && !test_hook("KC_NO_KEY_PASSES") && !test_hook("KC_NO_P3B") &&
        !test_hook("KC_NO_SORT_RUNS") && !test_hook("KC_NO_P5S_DIRECT")) {
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
            if (!kpass && sort_runs && records_empty(c) && c->stats_h[ST_CLAIMED] == 0 && b.n >= direct_min &&
                !test_hook("KC_NO_P5S_DIRECT")) {
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
    uint64_t max_reads = even_reads(L, std::max(safe_reads, skm_big_reads(c, nw, pool_cap)));
    safe_reads = even_reads(L, safe_reads);
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
            max_reads = even_reads(L, nr / 2);  // (nr >= 2: at least one read)
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
    const Engine e = engine_for(c, L);
    const bool sketch_skm = e == Engine::skm && !c->skm_force;
    // (the key-prefix engine: chosen, or the default engine's only one for this (L, k))
    const bool sketch_part = c->part && !c->count.hc_hint && e != Engine::skm;
    if ((sketch_skm || sketch_part) && !c->count.skm_checked && pre0 >= 0 && !test_hook("KC_NO_SKETCH") &&
        n_reads * (uint64_t)(L - c->k + 1) >= kSkmSampleMinKeys) {
        kc_status s = sketch_engine(c, n_reads, L, pre0);
        if (s) return s;
        if (sketch_part) c->count.skm_checked = true;  // once per reset
    }
    return KC_OK;
}

// Counts n_reads reads with the engine of engine_for, after the coverage sketch
// had its say. pre0 >= 0: the reads are pre-encoded in part_codes / part_inval
// from read pre0. The engines' common prologue and epilogue are here.
kc_status count_reads(kc_ctx* c, const uint8_t* base, const uint64_t* seq_off, uint64_t n_reads, int64_t L,
                      int64_t pre0) {
    if (c->count.finished) return fail(c, KC_ERR_STATE, "kc_finish was called; kc_reset first");
    kc_status s = sketch_gate(c, n_reads, L, pre0);
    if (s) return s;
    const Engine e = engine_for(c, L);
    if (e == Engine::table && pre0 >= 0) return fail(c, KC_ERR_INTERNAL, "pre-encoded reads reached the table engine");
    s = e == Engine::skm      ? count_reads_skm(c, base, seq_off, n_reads, L, skm_geometry((int)L, (int)c->k), pre0)
        : e == Engine::prefix ? count_reads_part(c, base, seq_off, n_reads, L, pre0)
                              : count_reads_table(c, base, seq_off, n_reads, L);
    if (s) return s;
    c->st.valid_kmers = c->stats_h[ST_VALID];
    c->st.spilled_kmers = c->count.spilled_flushed + c->stats_h[ST_SPILL_FILL];
    return KC_OK;
}

// Reads of length L one engine batch holds (its window capacity key_cap)
uint64_t batch_reads(const kc_ctx* c, int64_t L) {
    const uint64_t m = c->key_cap / (uint64_t)(L - c->k + 1);
    return m ? m : 1;
}

// Counts the n pre-encoded fixed-length reads of the pending batch, bs per
// count_reads call, with a run cut after each call when the records outgrow
// half the working set. More than one engine batch goes whole when it is a
// high-cardinality batch on an empty record state (key-range passes,
// count_reads_part); else by engine batches (the skm engine's may be large)
kc_status count_pending_fixed(kc_ctx* c, uint64_t n, int64_t L) {
    kc_status s;
    const uint64_t b = batch_reads(c, L);
    uint64_t bs = n;
    if (n > b) {
        if ((s = sketch_gate(c, n, L, 0))) return s;
        const bool passes = c->count.hc_hint && c->part && (!c->skm || c->count.skm_hc) && records_empty(c) &&
                            !test_hook("KC_NO_KEY_PASSES");
        if (!passes) {
            bs = b;
            if (engine_for(c, L) == Engine::skm)
                bs = std::max(b, skm_big_reads(c, (uint64_t)(L - c->k + 1), (uint64_t)c->W * c->key_cap / (c->W + 1)));
            bs = even_reads(L, bs);
        }
    }
    for (uint64_t r0 = 0; r0 < n; r0 += bs) {
        if ((s = count_reads(c, nullptr, nullptr, std::min(bs, n - r0), L, (int64_t)r0))) return s;
        if ((s = cut_run_if_full(c))) return s;
    }
    return KC_OK;
}
