// kc_finish.cpp — everything that turns records into the finished, sorted,
// packed run: the radix sort of SoA records, the spill runs, the engines'
// finishes (kc_finish), cut runs, the merges of packed runs (one device, many).
#include <errno.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <thread>

#include "kc_ctx.h"

// ---------------------------------------------------------------------------
// sorting helpers (device)
// ---------------------------------------------------------------------------

// Sorts n SoA records (keys at `stride`) in place-or-swap; returns which buffer
// holds the result (0 = a, 1 = b).
kc_status sort_records(kc_ctx* c, uint64_t* ka, uint64_t* kb, uint32_t* va, uint32_t* vb, uint64_t stride, uint64_t n,
                       int* which, int words) {
    *which = 0;
    if (n <= 1) return KC_OK;
    const int W = words ? words : c->W;
    kc_status s = ensure(c, c->fin_misc, 2 * W * 8);
    if (s) return s;
    std::vector<uint64_t> init(2 * W);
    for (int j = 0; j < W; j++) {
        init[j] = 0;
        init[W + j] = ~0ull;
    }
    HIPCHK(c, hipMemcpyAsync(c->fin_misc.p, init.data(), 2 * W * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_key_bits(W, ka, stride, n, c->fin_misc.as<uint64_t>(), c->stream));
    std::vector<uint64_t> bits(2 * W);
    HIPCHK(c, hipMemcpyAsync(bits.data(), c->fin_misc.p, 2 * W * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int grid = sort_grid(n);
    s = ensure(c, c->fin_hist, (size_t)sort_hist_elems(grid) * 8);
    if (s) return s;
    uint64_t* kin = ka;
    uint64_t* kout = kb;
    uint32_t* vin = va;
    uint32_t* vout = vb;
    int cur = 0;
    for (int word = W - 1; word >= 0; word--) {
        uint64_t vary = bits[word] ^ bits[W + word];
        for (int shift = 0; shift < 64; shift += 8) {
            if (((vary >> shift) & 255u) == 0) continue;
            HIPCHK(c, launch_sort_pass(W, kin, kout, vin, vout, stride, n, word, shift, c->fin_hist.as<uint64_t>(),
                                       grid, false, c->stream));
            std::swap(kin, kout);
            std::swap(vin, vout);
            cur ^= 1;
        }
    }
    *which = cur;
    return KC_OK;
}

// ---------------------------------------------------------------------------
// spill runs: sort the spill buffer, run-length reduce, pack, move to host
// ---------------------------------------------------------------------------

// A sorted packed run of n records (device memory, rewritten later) kept as a
// device run when HBM has room for it plus a margin; false: the caller keeps
// it on the host.
static bool keep_run_on_device(kc_ctx* c, const void* packed, uint64_t n) {
    const size_t bytes = (size_t)n * c->rs;
    size_t mfree = 0, mtotal = 0;
    DevBuf run;
    if (test_hook("KC_HOST_RUNS")) return false;  // tests: runs leave HBM as they do when it is short
    if (hipMemGetInfo(&mfree, &mtotal) != hipSuccess || mfree < bytes + ((size_t)4 << 30) ||
        run.alloc(bytes ? bytes : 16) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    run.bytes = bytes;  // (0 for an empty run: the pool never hands it out)
    if (hipMemcpyAsync(run.p, packed, bytes, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    c->dev_runs.push_back(std::move(run));
    c->dev_run_n.push_back(n);
    c->count.runs_cut++;
    return true;
}

// n >= 1 sorted keys (SoA at `stride`): the heads of the runs of equal keys
// flagged in rle_flags, the flags scanned into rle_pos (both grown here, with
// the scan's scratch), and the last position and flag on their way back into
// last[0..1]. Does not synchronise: once the caller has, last[0] + last[1] is
// the number of distinct keys.
static kc_status rle_heads_scan(kc_ctx* c, const uint64_t* keys, uint64_t stride, uint64_t n, uint32_t* last) {
    kc_status s;
    if ((s = ensure(c, c->rle_flags, n * 4)) || (s = ensure(c, c->rle_pos, n * 4)) ||
        (s = ensure(c, c->rle_tmp, scan_tmp_elems(n) * 4)))
        return s;
    HIPCHK(c, launch_rle_heads(c->W, keys, stride, n, c->rle_flags.as<uint32_t>(), c->stream));
    HIPCHK(c, launch_scan_u32(c->rle_flags.as<uint32_t>(), c->rle_pos.as<uint32_t>(), n, c->rle_tmp.as<uint32_t>(),
                              c->stream));
    HIPCHK(c, hipMemcpyAsync(&last[0], c->rle_pos.as<uint32_t>() + (n - 1), 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&last[1], c->rle_flags.as<uint32_t>() + (n - 1), 4, hipMemcpyDeviceToHost, c->stream));
    return KC_OK;
}

// Sorts n spilled keys (SoA at `stride` in `keys`, `scratch` of the same
// shape), run-length reduces them and stores the run (host memory or a temp
// file).
static kc_status flush_keys(kc_ctx* c, uint64_t* keys, uint64_t stride, uint64_t n, uint64_t* scratch) {
    kc_status s;
    const int W = c->W;
    int which = 0;
    if ((s = sort_records(c, keys, scratch, nullptr, nullptr, stride, n, &which))) return s;
    uint64_t* sorted = which ? scratch : keys;
    uint32_t last[2];
    if ((s = ensure(c, c->rle_head, n * 4)) || (s = ensure(c, c->run_keys, (size_t)W * n * 8)) ||
        (s = ensure(c, c->run_cnts, n * 4)) || (s = rle_heads_scan(c, sorted, stride, n, last)))
        return s;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t m = (uint64_t)last[0] + last[1];
    HIPCHK(c, launch_rle_scatter(W, sorted, stride, n, c->rle_flags.as<uint32_t>(), c->rle_pos.as<uint32_t>(),
                                 c->run_keys.as<uint64_t>(), n, c->rle_head.as<uint32_t>(), c->stream));
    HIPCHK(c, launch_rle_counts(c->rle_head.as<uint32_t>(), m, n, c->run_cnts.as<uint32_t>(), c->stream));
    size_t bytes = (size_t)m * c->rs;
    if ((s = ensure(c, c->run_packed, bytes))) return s;
    HIPCHK(c, launch_pack(W, c->run_keys.as<uint64_t>(), n, c->run_cnts.as<uint32_t>(), m, c->run_packed.p, c->stream));
    c->count.spilled_flushed += n;
    // the run stays in HBM (merged on the device by kc_finish) unless HBM is
    // short: then host memory, or a file in tempFileLocation
    if (keep_run_on_device(c, c->run_packed.p, m)) return KC_OK;
    HostRun run;
    run.records = m;
    run.mem.resize(bytes);
    HIPCHK(c, hipMemcpyAsync(run.mem.data(), c->run_packed.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!c->temp_dir.empty()) {
        char name[128];
        snprintf(name, sizeof(name), "/kc.%d.%llu.%zu", (int)getpid(), (unsigned long long)c->id, c->runs.size());
        run.path = c->temp_dir + name;
        FILE* f = fopen(run.path.c_str(), "wb");
        if (!f) return fail(c, KC_ERR_IO, "cannot create spill run %s: %s", run.path.c_str(), strerror(errno));
        size_t w = fwrite(run.mem.data(), 1, bytes, f);
        const int we = errno;
        const int ce = fclose(f) != 0 ? errno : 0;
        if (w != bytes || ce)
            return fail(c, KC_ERR_IO, "short write to spill run %s (%zu of %llu bytes): %s", run.path.c_str(), w,
                        (unsigned long long)bytes, strerror(w != bytes ? we : ce));
        std::vector<uint8_t>().swap(run.mem);
    }
    c->runs.push_back(std::move(run));
    c->st.spill_runs = c->runs.size();
    return KC_OK;
}

// Flushes the spill buffer of the global table into a sorted run.
kc_status flush_spill(kc_ctx* c) {
    kc_status s = sync_stats(c);
    if (s) return s;
    uint64_t n = c->stats_h[ST_SPILL_FILL];
    if (n == 0) return KC_OK;
    if (n > c->spill_cap) return fail(c, KC_ERR_INTERNAL, "spill buffer overflow (%llu > %llu)",
                                      (unsigned long long)n, (unsigned long long)c->spill_cap);
    if ((s = ensure(c, c->spill_keys2, (size_t)c->W * c->spill_cap * 8))) return s;
    if ((s = flush_keys(c, c->spill, c->spill_cap, n, c->spill_keys2.as<uint64_t>()))) return s;
    HIPCHK(c, hipMemsetAsync(c->stats + ST_SPILL_FILL, 0, 8, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stats_h[ST_SPILL_FILL] = 0;
    return KC_OK;
}

// After a batch's P5 (statistics synchronised): the keys it spilled into the
// free key buffer `spill` (ST_SPILL2_FILL of them, SoA at key_cap; `scratch`:
// the other key buffer) become a sorted run
kc_status flush_spill2(kc_ctx* c, uint64_t* spill, uint64_t* scratch) {
    kc_status s;
    if (c->stats_h[ST_ERR] & ERR_SPILL_OVERFLOW) return fail(c, KC_ERR_INTERNAL, "spill buffer overflow");
    const uint64_t n2 = c->stats_h[ST_SPILL2_FILL];
    if (n2 == 0) return KC_OK;
    if ((s = flush_keys(c, spill, c->key_cap, n2, scratch))) return s;
    HIPCHK(c, hipMemsetAsync(c->stats + ST_SPILL2_FILL, 0, 8, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stats_h[ST_SPILL2_FILL] = 0;
    return KC_OK;
}

// The SoA finish buffers fin_keys[i] / fin_cnts[i] hold out_cap records of W
// key words each, for i < nbuf: both ping-pong buffers, or buffer 0 alone.
static kc_status ensure_fin(kc_ctx* c, uint64_t out_cap, int nbuf = 2) {
    kc_status s;
    for (int i = 0; i < nbuf; i++) {
        if ((s = ensure(c, c->fin_keys[i], (size_t)c->W * out_cap * 8)) || (s = ensure(c, c->fin_cnts[i], out_cap * 4)))
            return s;
    }
    return KC_OK;
}

// Appends the global table's records and then key 0 (when present) behind the
// nrec records of keys / cnts (SoA at `stride`); *n receives the record count
// (read back: synchronises). The cursor is fin_misc word 2W, the compaction's
// scratch follows it (the caller sized fin_misc). With `t` the table is
// compacted only when it claimed slots and *t receives its record count (one
// more read-back and wait); without `t` (the table engine, nrec == 0) it is
// always compacted and that count stays on the device.
static kc_status append_table_key0(kc_ctx* c, uint64_t* keys, uint32_t* cnts, uint64_t stride, uint64_t nrec,
                                   uint64_t* t, uint64_t* n) {
    uint64_t* cursor = c->fin_misc.as<uint64_t>() + 2 * c->W;
    uint64_t cur = nrec;  // (kept alive until the stream is synchronised below)
    if (!t || c->stats_h[ST_CLAIMED])
        HIPCHK(c, launch_compact(c->W, c->table, c->cap, keys + nrec, cnts + nrec, stride, cursor, cursor + 1,
                                 c->stream));
    if (t) {
        *t = 0;
        if (c->stats_h[ST_CLAIMED]) {
            HIPCHK(c, hipMemcpyAsync(t, cursor, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        cur += *t;
        HIPCHK(c, hipMemcpyAsync(cursor, &cur, 8, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, launch_append_key0(c->W, keys, cnts, stride, cursor, c->stats, c->stream));
    HIPCHK(c, hipMemcpyAsync(n, cursor, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KC_OK;
}

// After launch_seg_sort: reads the statistics back (synchronises); a segment
// beyond the LDS sort's capacity is an internal error.
static kc_status seg_sort_check(kc_ctx* c) {
    const kc_status s = sync_stats(c);
    if (s) return s;
    if (c->stats_h[ST_ERR] & ERR_SEG_TOO_LONG) return fail(c, KC_ERR_INTERNAL, "segment longer than its LDS sort");
    return KC_OK;
}

// The context is finished with the n records in fin_packed. The merges close
// their timing here: the time since mk.begin(), waited for, goes to finish_ms.
static kc_status finished_with(kc_ctx* c, Marks& mk, uint64_t n) {
    HIPCHK(c, mk.mark());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, mk.add(0, c->st.finish_ms));
    c->count.n_records = n;
    c->st.output_records = n;
    c->count.finished = true;
    return KC_OK;
}

// fin_keys[which]/fin_cnts[which] hold n sorted records (equal keys adjacent):
// sum equal keys (segmented reduce) when `dups`, pack into fin_packed.
static kc_status reduce_pack(kc_ctx* c, uint64_t out_cap, uint64_t n, int which, bool dups, uint64_t* n_out) {
    kc_status s;
    const int W = c->W;
    if (dups && n > 1) {
        uint64_t* ks = c->fin_keys[which].as<uint64_t>();
        uint32_t* cs = c->fin_cnts[which].as<uint32_t>();
        uint64_t* ko = c->fin_keys[which ^ 1].as<uint64_t>();
        uint32_t* co = c->fin_cnts[which ^ 1].as<uint32_t>();
        uint32_t last[2];
        if ((s = rle_heads_scan(c, ks, out_cap, n, last))) return s;
        HIPCHK(c, hipMemsetAsync(co, 0, n * 4, c->stream));
        HIPCHK(c, launch_reduce_add(W, ks, out_cap, cs, n, c->rle_flags.as<uint32_t>(), c->rle_pos.as<uint32_t>(), ko,
                                    out_cap, co, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        n = (uint64_t)last[0] + last[1];
        which ^= 1;
    }
    if ((s = ensure(c, c->fin_packed, (size_t)n * c->rs + 16))) return s;
    HIPCHK(c, launch_pack(W, c->fin_keys[which].as<uint64_t>(), out_cap, c->fin_cnts[which].as<uint32_t>(), n,
                          c->fin_packed.p, c->stream));
    *n_out = n;
    return KC_OK;
}

// fin_keys[0]/fin_cnts[0] hold n records at stride out_cap: radix sort, sum
// equal keys when `dups` may exist, pack into fin_packed.
static kc_status sort_reduce_pack(kc_ctx* c, uint64_t out_cap, uint64_t n, bool dups, uint64_t* n_out) {
    kc_status s;
    uint64_t* k0 = c->fin_keys[0].as<uint64_t>();
    uint32_t* c0 = c->fin_cnts[0].as<uint32_t>();
    int which = 0;
    if ((s = sort_records(c, k0, c->fin_keys[1].as<uint64_t>(), c0, c->fin_cnts[1].as<uint32_t>(), out_cap, n, &which)))
        return s;
    return reduce_pack(c, out_cap, n, which, dups, n_out);
}

// Sorted finish of the partition engine (one batch, every key counted in LDS):
// the records of each P5 pass form one key-ordered segment; the descriptors
// (bucket << 48 | first key fraction) are sorted, their lengths scanned into
// output offsets, and seg_sort sorts every segment into place. Key 0, the
// smallest key, goes first. No global radix sort.
static kc_status finish_part_sorted(kc_ctx* c, uint64_t ndesc, uint64_t* n_out) {
    kc_status s;
    const int W = c->W;
    const uint64_t nrec = c->count.rec_n;
    const bool key0 = c->stats_h[ST_KEY0_PRESENT] != 0;
    const uint64_t off0 = key0 ? 1 : 0;
    const uint64_t n = nrec + off0;
    const uint64_t out_cap = n + 1;
    if ((s = ensure_fin(c, out_cap, 1))) return s;  // buffer 0 only: seg_sort writes the packed output
    uint64_t* k0 = c->fin_keys[0].as<uint64_t>();
    uint32_t* c0 = c->fin_cnts[0].as<uint32_t>();
    if (ndesc) {
        if ((s = ensure(c, c->desc_k2, ndesc * 8)) || (s = ensure(c, c->desc_v, ndesc * 4)) ||
            (s = ensure(c, c->desc_v2, ndesc * 4)) || (s = ensure(c, c->desc_lens, ndesc * 8)) ||
            (s = ensure(c, c->desc_offs, ndesc * 8)) || (s = ensure(c, c->rle_tmp, scan_tmp_elems(ndesc) * 8)))
            return s;
        // KC_TRACE: each phase synchronised and timed
        double tp = kc::trace_on() ? kc::now_s() : 0;
        auto phase = [&](const char* what) {
            if (!kc::trace_on()) return;
            if (hipStreamSynchronize(c->stream) != hipSuccess) return;
            const double t = kc::now_s();
            kc::trace("finish_part_sorted %s: %.3f ms", what, (t - tp) * 1e3);
            tp = t;
        };
        phase("buffers");
        HIPCHK(c, launch_iota_u32(c->desc_v.as<uint32_t>(), ndesc, c->stream));
        int which = 0;
        if ((s = sort_records(c, c->desc_key.as<uint64_t>(), c->desc_k2.as<uint64_t>(), c->desc_v.as<uint32_t>(),
                              c->desc_v2.as<uint32_t>(), ndesc, ndesc, &which, 1)))
            return s;
        phase("descriptor sort");
        const uint32_t* order = (which ? c->desc_v2 : c->desc_v).as<uint32_t>();
        HIPCHK(c, launch_desc_prep(order, c->desc_len.as<uint32_t>(), ndesc, c->desc_lens.as<uint64_t>(),
                                   c->stream));
        HIPCHK(c, launch_scan_u64(c->desc_lens.as<uint64_t>(), c->desc_offs.as<uint64_t>(), ndesc,
                                  c->rle_tmp.as<uint64_t>(), c->stream));
        // LSD fallback list (u32 per descriptor + count) in the free sort scratch
        if ((s = ensure(c, c->desc_fb, ndesc * 4 + 16))) return s;
        uint32_t* fb = c->desc_fb.as<uint32_t>();
        uint64_t* fb_n = c->desc_lens.as<uint64_t>();  // desc_lens is consumed by the scan above
        // sorted straight into the packed output, after the key-0 record
        if ((s = ensure_pooled(c, c->fin_packed, (size_t)n * c->rs + 16))) return s;
        phase("descriptor scan");
        DescSink desc = desc_sink(c);
        desc.key = (which ? c->desc_k2 : c->desc_key).as<uint64_t>();  // the sorted descriptor keys
        HIPCHK(c, launch_seg_sort(W, rec_sink(c), order, desc, c->desc_offs.as<uint64_t>(), ndesc,
                                  {k0 + off0, c0 + off0, out_cap, nullptr}, c->stats, fb, fb_n, c->n_cu, c->stream,
                                  c->fin_packed.as<char>() + off0 * c->rs));
        phase("segment sort");
    }
    if ((s = ensure_pooled(c, c->fin_packed, (size_t)n * c->rs + 16))) return s;
    // record 0: key 0^W (all-zero words) and its count (kept alive until the
    // stream is synchronised below)
    std::vector<uint32_t> r0((size_t)c->rs / 4, 0u);
    if (key0) {
        r0.back() = (uint32_t)c->stats_h[ST_KEY0];
        HIPCHK(c, hipMemcpyAsync(c->fin_packed.p, r0.data(), c->rs, hipMemcpyHostToDevice, c->stream));
    }
    if ((s = seg_sort_check(c))) return s;
    *n_out = n;
    return KC_OK;
}

// Finish whenever an skm batch contributed: the P5 records (+ global-table
// records + key 0) are grouped by their first 8 bases (word0 >> 48) with the
// rp_* passes (counts as payload), every group is sorted in LDS by seg_sort_k,
// equal keys (several batches, the global table) are summed, then packed. A
// group longer than seg_sort's capacity (skewed keys) or a small record set
// takes the global radix sort instead.
static kc_status finish_skm(kc_ctx* c, uint64_t* n_out) {
    kc_status s;
    const int W = c->W;
    const uint64_t nrec = c->count.rec_n;
    const uint64_t claimed = c->stats_h[ST_CLAIMED];
    if ((s = grow_records(c, nrec + claimed + 1))) return s;
    if ((s = ensure(c, c->fin_misc, (2 * W + 2 + compact_tmp_elems()) * 8))) return s;
    uint64_t* longest = c->fin_misc.as<uint64_t>() + 2 * W + 1 + compact_tmp_elems();
    uint64_t t = 0, n = 0;
    if ((s = append_table_key0(c, c->rec_keys, c->rec_cnts, c->rec_cap, nrec, &t, &n))) return s;
    const bool dups = c->count.batches > 1 || t > 0;
    const uint64_t out_cap = n + 1;
    if ((s = ensure_fin(c, out_cap))) return s;
    uint64_t* k0 = c->fin_keys[0].as<uint64_t>();
    uint32_t* c0 = c->fin_cnts[0].as<uint32_t>();
    const uint32_t nb = 1u << kBucketBits;
    bool grouped = n >= nb && n <= c->key_cap && !test_hook("KC_NO_SEGSORT");
    if (grouped) {
        // only the skm engine wrote records since the reset: P5 wrote their
        // first grouping digit (rec_dig), the table's and key 0's (appended
        // above) are added here, and the first pass reads 1 B per record
        const bool dig1 = c->count.engines_used == 1 && c->rec_dig && !test_hook("KC_NO_REC_DIG");
        if (dig1 && n > nrec)
            HIPCHK(c, launch_key_digits(c->rec_keys, nrec, n, 48, c->rec_dig, c->stream));
        double gm[2] = {0, 0};
        if ((s = group16(c, W, true, c->rec_keys, c->rec_cap, c->rec_cnts, c->fin_keys[1].as<uint64_t>(), out_cap,
                         c->fin_cnts[1].as<uint32_t>(), c->digs, n, gm, dig1 ? c->rec_dig.as<uint8_t>() : nullptr)))
            return s;
        c->count.finish_group_ms += gm[0] + gm[1];
        if ((s = ensure(c, c->part_starts, ((size_t)nb + 1) * 8)) || (s = ensure(c, c->desc_v, (size_t)nb * 4)) ||
            (s = ensure(c, c->desc_len, (size_t)nb * 4)) || (s = ensure(c, c->desc_fb, (size_t)nb * 4 + 16)))
            return s;
        HIPCHK(c, launch_bucket_bounds(W, c->rec_keys, c->rec_cap, n, kBucketBits, c->part_starts.as<uint64_t>(),
                                       c->stream));
        // the groups' descriptors (digit: word0 bits 36..47, the 12 bits below
        // the 16-bit group prefix) built on the device; only the longest
        // group's length comes back
        HIPCHK(c, hipMemsetAsync(longest, 0, 8, c->stream));
        HIPCHK(c, launch_group_desc(c->part_starts.as<uint64_t>(), nb, 36u, c->desc_v.as<uint32_t>(),
                                    c->desc_len.as<uint32_t>(), longest, c->stream));
        uint64_t mx = 0;
        HIPCHK(c, hipMemcpyAsync(&mx, longest, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (mx > (uint64_t)seg_sort_cap(W)) grouped = false;
    }
    if (grouped) {
        uint64_t* fb_n = (uint64_t*)(c->desc_fb.as<char>() + (size_t)nb * 4);
        // one batch, no table records: keys are distinct, so the groups are
        // sorted straight into the packed output
        if (!dups && (s = ensure(c, c->fin_packed, (size_t)n * c->rs + 16))) return s;
        // every group a segment, sorted where it stands: the bucket bounds are its start and its output offset
        const DescSink groups = {nullptr, c->part_starts.as<uint64_t>(), c->desc_len.as<uint32_t>(), nb};
        HIPCHK(c, launch_seg_sort(W, rec_sink(c), c->desc_v.as<uint32_t>(), groups, c->part_starts.as<uint64_t>(), nb,
                                  {k0, c0, out_cap, nullptr}, c->stats, c->desc_fb.as<uint32_t>(), fb_n, c->n_cu,
                                  c->stream, dups ? nullptr : c->fin_packed.p));
        if ((s = seg_sort_check(c))) return s;
        if (!dups) {
            *n_out = n;
            return KC_OK;
        }
        return reduce_pack(c, out_cap, n, 0, dups, n_out);
    }
    if (n) {
        for (int j = 0; j < W; j++)
            HIPCHK(c, hipMemcpyAsync(k0 + (size_t)j * out_cap, c->rec_keys + (size_t)j * c->rec_cap, n * 8,
                                     hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c0, c->rec_cnts, n * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    return sort_reduce_pack(c, out_cap, n, dups, n_out);
}

// Finish of the partition engine: LDS records + fallback-table records + key 0
// -> radix sort -> (sum duplicates when several batches or the fallback table
// contributed) -> pack.
static kc_status finish_part(kc_ctx* c, uint64_t* n_out) {
    if (c->count.skm_used) return finish_skm(c, n_out);
    kc_status s;
    const int W = c->W;
    const uint64_t nrec = c->count.rec_n;
    const uint64_t claimed = c->stats_h[ST_CLAIMED];
    const uint64_t ndesc = c->stats_h[ST_DESC_FILL];
    kc::trace("finish_part: %llu records, %llu batches, %llu claimed, %zu host runs, %llu descriptors",
              (unsigned long long)nrec, (unsigned long long)c->count.batches, (unsigned long long)claimed, c->runs.size(),
              (unsigned long long)ndesc);
    if (c->count.batches <= 1 && claimed == 0 && c->runs.empty() && ndesc <= kDescCap && !test_hook("KC_NO_SEGSORT"))
        return finish_part_sorted(c, ndesc, n_out);
    const uint64_t out_cap = nrec + claimed + 1;
    if ((s = ensure_fin(c, out_cap))) return s;
    if ((s = ensure(c, c->fin_misc, (2 * W + 1 + compact_tmp_elems()) * 8))) return s;
    uint64_t* k0 = c->fin_keys[0].as<uint64_t>();
    uint32_t* c0 = c->fin_cnts[0].as<uint32_t>();
    if (nrec) {
        for (int j = 0; j < W; j++)
            HIPCHK(c, hipMemcpyAsync(k0 + (size_t)j * out_cap, c->rec_keys + (size_t)j * c->rec_cap, nrec * 8,
                                     hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c0, c->rec_cnts, nrec * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    uint64_t t = 0, n = 0;
    if ((s = append_table_key0(c, k0, c0, out_cap, nrec, &t, &n))) return s;
    return sort_reduce_pack(c, out_cap, n, c->count.batches > 1 || t > 0, n_out);
}

// Table engine: the global table compacted, radix-sorted and packed into
// fin_packed (key 0 first when present).
static kc_status finish_table(kc_ctx* c, uint64_t* n_out) {
    kc_status s;
    const int W = c->W;
    uint64_t out_cap = c->stats_h[ST_CLAIMED] + 1;
    if ((s = ensure_fin(c, out_cap))) return s;
    if ((s = ensure(c, c->fin_misc, (2 * W + 1 + compact_tmp_elems()) * 8))) return s;
    uint64_t n = 0;
    if ((s = append_table_key0(c, c->fin_keys[0].as<uint64_t>(), c->fin_cnts[0].as<uint32_t>(), out_cap, 0, nullptr, &n)))
        return s;
    if (n > out_cap) return fail(c, KC_ERR_INTERNAL, "compaction found %llu records, expected <= %llu",
                                 (unsigned long long)n, (unsigned long long)out_cap);
    int which = 0;
    // note: sort_records re-uses fin_misc for the key bits (cursor already read)
    if ((s = sort_records(c, c->fin_keys[0].as<uint64_t>(), c->fin_keys[1].as<uint64_t>(), c->fin_cnts[0].as<uint32_t>(),
                          c->fin_cnts[1].as<uint32_t>(), out_cap, n, &which)))
        return s;
    if ((s = ensure(c, c->fin_packed, (size_t)n * c->rs + 16))) return s;
    HIPCHK(c, launch_pack(W, c->fin_keys[which].as<uint64_t>(), out_cap, c->fin_cnts[which].as<uint32_t>(), n,
                          c->fin_packed.p, c->stream));
    *n_out = n;
    return KC_OK;
}

// One sorted packed run of n records (n may be 0) that may repeat keys, equal
// keys adjacent -> the ctx's finished table run: unpacked into SoA keys, equal
// neighbours summed (u32, wrapping), packed into fin_packed.
static kc_status merge_one_run(kc_ctx* c, const void* run, uint64_t n) {
    kc_status s;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const uint64_t out_cap = n + 1;
    if ((s = ensure_fin(c, out_cap))) return s;
    Marks mk{c};
    HIPCHK(c, mk.begin());
    if (n)
        HIPCHK(c, launch_unpack(c->W, run, n, c->fin_keys[0].as<uint64_t>(), out_cap, c->fin_cnts[0].as<uint32_t>(),
                                c->stream));
    uint64_t nout = 0;
    if ((s = reduce_pack(c, out_cap, n, 0, true, &nout))) return s;
    return finished_with(c, mk, nout);
}

// Sorted runs without repeated keys (kc_finish output, cut runs, slices of
// them) -> the finished table run: pairwise merge path over the packed
// records, level by level (launch_merge_packed), into ping-pong buffers; keys
// present in several runs come out as adjacent records and are summed after
// the last level (SoA segmented reduce). One run is taken as it is.
static kc_status merge_runs_packed(kc_ctx* c, const std::vector<std::pair<const void*, uint64_t>>& runs0) {
    kc_status s;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    std::vector<std::pair<const void*, uint64_t>> runs;
    uint64_t n = 0;
    for (auto& r : runs0)
        if (r.second) {
            runs.push_back(r);
            n += r.second;
        }
    const size_t rs = (size_t)c->rs;
    Marks mk{c};
    HIPCHK(c, mk.begin());
    if ((s = ensure(c, c->fin_misc, (merge_packed_split_elems(c->W, n) + 8) * 8))) return s;
    uint32_t* dup = (uint32_t*)(c->fin_misc.as<uint64_t>() + merge_packed_split_elems(c->W, n) + 2);
    uint64_t* split = c->fin_misc.as<uint64_t>();
    HIPCHK(c, hipMemsetAsync(dup, 0, 4, c->stream));
    if (runs.size() <= 1) {
        if ((s = ensure_pooled(c, c->fin_packed, n * rs + 16))) return s;
        if (n && runs[0].first != c->fin_packed.p)
            HIPCHK(c, hipMemcpyAsync(c->fin_packed.p, runs[0].first, n * rs, hipMemcpyDeviceToDevice, c->stream));
    } else {
        DevBuf* out[2] = {&c->fin_packed, &c->merge_tmp};
        int lvl = 0;
        while (runs.size() > 1) {
            DevBuf* o = out[lvl & 1];
            if ((s = ensure_pooled(c, *o, n * rs + 16))) return s;
            std::vector<std::pair<const void*, uint64_t>> next;
            uint64_t off = 0;
            for (size_t r = 0; r < runs.size(); r += 2) {
                uint8_t* dst = (uint8_t*)o->p + off * rs;
                if (r + 1 < runs.size()) {
                    HIPCHK(c, launch_merge_packed(c->W, runs[r].first, runs[r].second, runs[r + 1].first,
                                                  runs[r + 1].second, dst, split, dup, c->stream));
                    next.push_back({dst, runs[r].second + runs[r + 1].second});
                } else {
                    HIPCHK(c, hipMemcpyAsync(dst, runs[r].first, runs[r].second * rs, hipMemcpyDeviceToDevice,
                                             c->stream));
                    next.push_back({dst, runs[r].second});
                }
                off += next.back().second;
            }
            runs.swap(next);
            lvl++;
        }
        if (runs[0].first != c->fin_packed.p) std::swap(c->fin_packed, c->merge_tmp);
    }
    uint32_t dup_h = 0;
    HIPCHK(c, hipMemcpyAsync(&dup_h, dup, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t nout = n;
    if (dup_h) {
        // keys of several runs: sum them (unpack, segmented reduce, pack)
        const uint64_t out_cap = n + 1;
        if ((s = ensure_fin(c, out_cap))) return s;
        HIPCHK(c, launch_unpack(c->W, c->fin_packed.p, n, c->fin_keys[0].as<uint64_t>(), out_cap,
                                c->fin_cnts[0].as<uint32_t>(), c->stream));
        if ((s = reduce_pack(c, out_cap, n, 0, true, &nout))) return s;
    }
    return finished_with(c, mk, nout);
}

kc_status kc_finish(kc_ctx* c, uint64_t* n_records) {
    if (!c) return KC_ERR_ARG;
    if (c->count.finished) {
        if (n_records) *n_records = c->count.n_records;
        return KC_OK;
    }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    kc_status s;
    c->count.ckpt = false;
    if (c->acc_t[3] > 0) {
        kc::trace("chunk calls %.0f: host copy %.3f ms, buffer waits %.3f ms, flushes %.3f ms", c->acc_t[3],
                  c->acc_t[0] * 1e3, c->acc_t[1] * 1e3, c->acc_t[2] * 1e3);
        for (double& x : c->acc_t) x = 0;
    }
    if ((s = pend_flush(c))) return s;
    if ((s = sync_stats(c))) return s;
    if (c->stats_h[ST_SPILL_FILL] > 0 && (s = flush_spill(c))) return s;
    // the table run: the engines' records (or the global table) sorted into fin_packed
    // (own events: the grouping passes inside record ev0..ev2 themselves)
    HIPCHK(c, hipEventRecord(c->evf[0], c->stream));
    uint64_t n = 0;
    if ((s = c->part ? finish_part(c, &n) : finish_table(c, &n))) return s;
    HIPCHK(c, hipEventRecord(c->evf[1], c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float tf = 0.f;
    HIPCHK(c, hipEventElapsedTime(&tf, c->evf[0], c->evf[1]));
    c->st.finish_ms += tf;
    c->st.table_used = c->stats_h[ST_CLAIMED];
    if (c->dev_runs.size() == 1 && n == 0) {
        // one sorted run and no table run (key-range passes, one direct
        // batch): the run is the output, its buffer becomes fin_packed
        if (c->fin_packed.p) c->run_pool.push_back(std::move(c->fin_packed));
        c->fin_packed = std::move(c->dev_runs[0]);
        n = c->dev_run_n[0];
        c->dev_runs.clear();
        c->dev_run_n.clear();
    }
    if (!c->dev_runs.empty()) {
        // sorted runs in HBM (cut runs, spill runs): the table run joins them
        // (taking over fin_packed's buffer), one merge of all
        std::vector<std::pair<const void*, uint64_t>> runs;
        for (size_t r = 0; r < c->dev_runs.size(); r++) runs.push_back({c->dev_runs[r].p, c->dev_run_n[r]});
        DevBuf table_run;
        if (n) {
            table_run = take_fin_packed(c);
            runs.push_back({table_run.p, n});
        }
        const double tm = kc::trace_on() ? kc::now_s() : 0;
        s = merge_runs_packed(c, runs);
        kc::trace("merge of %zu runs: %.3f ms", runs.size(), (kc::now_s() - tm) * 1e3);
        if (table_run.p) c->run_pool.push_back(std::move(table_run));
        release_dev_runs(c);
        if (s) return s;
        if (n_records) *n_records = c->count.n_records;
        return KC_OK;
    }
    c->count.n_records = n;
    c->count.finished = true;
    c->st.output_records = n;
    if (n_records) *n_records = n;
    return KC_OK;
}

kc_status kc_merge_records_device(kc_ctx* c, const void* d_packed, uint64_t n_records) {
    if (!c || (!d_packed && n_records)) return KC_ERR_ARG;
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    if (!c->runs.empty()) return fail(c, KC_ERR_STATE, "spill runs exist");
    kc_status s;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const uint64_t out_cap = n_records + 1;
    if ((s = ensure_fin(c, out_cap))) return s;
    Marks mk{c};
    HIPCHK(c, mk.begin());
    HIPCHK(c, launch_unpack(c->W, d_packed, n_records, c->fin_keys[0].as<uint64_t>(), out_cap,
                            c->fin_cnts[0].as<uint32_t>(), c->stream));
    uint64_t n = 0;
    if ((s = sort_reduce_pack(c, out_cap, n_records, true, &n))) return s;
    return finished_with(c, mk, n);
}

// kc_canonicalize's work on a finished run of n >= 1 records. The staying
// records (cleared keys) go in order into `stay`: an ascending run, equal keys
// adjacent (clearing low bits keeps an ascending sequence ascending). The
// flipped ones go to SoA with their reverse-complement keys, are radix-sorted,
// summed and packed into fin_packed (the source run: every launch that reads
// it is ahead of the pack on the stream), which then leaves as `flip`. The two
// runs are merged; keys that meet are summed after the merge. The caller
// retires `stay` and `flip`.
static kc_status canon_fold(kc_ctx* c, uint64_t n, DevBuf& stay, DevBuf& flip) {
    kc_status s;
    const uint64_t ntiles = (n + filter_tile() - 1) / filter_tile();
    // tile counts, their exclusive scan, the total, the scan's scratch
    if ((s = ensure(c, c->q_tiles, (2 * ntiles + scan_tmp_elems(ntiles) + 1) * 8))) return s;
    uint64_t* cnt = c->q_tiles.as<uint64_t>();
    uint64_t* base = cnt + ntiles;
    uint64_t* total = base + ntiles;
    uint64_t* tmp = total + 1;
    Marks mk{c};
    HIPCHK(c, mk.begin());
    HIPCHK(c, launch_canon_count(c->fin_packed.p, c->W, (int)c->k, n, cnt, c->stream));
    HIPCHK(c, launch_scan_u64(cnt, base, ntiles, tmp, c->stream));
    HIPCHK(c, launch_sum_last(base, cnt, ntiles, total, c->stream));
    uint64_t n_stay = 0;
    HIPCHK(c, hipMemcpyAsync(&n_stay, total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_stay > n) return fail(c, KC_ERR_INTERNAL, "canonical fold kept %llu of %llu records", (unsigned long long)n_stay,
                                (unsigned long long)n);
    const uint64_t n_flip = n - n_stay;
    const uint64_t out_cap = n_flip + 1;
    if ((s = ensure_fin(c, out_cap, n_flip ? 2 : 1)) || (s = ensure_pooled(c, stay, (size_t)n_stay * c->rs + 16)))
        return s;
    HIPCHK(c, launch_canon_split(c->fin_packed.p, c->W, (int)c->k, n, base, stay.p, c->fin_keys[0].as<uint64_t>(),
                                 out_cap, c->fin_cnts[0].as<uint32_t>(), c->stream));
    kc::trace("canonical fold: %llu records, %llu stay, %llu flipped", (unsigned long long)n,
              (unsigned long long)n_stay, (unsigned long long)n_flip);
    uint64_t nf = 0;
    if (n_flip && (s = sort_reduce_pack(c, out_cap, n_flip, true, &nf))) return s;
    // the flipped run alone is the result
    if (n_stay == 0) return finished_with(c, mk, nf);
    // the merges time themselves (they restart the marks): close this part
    HIPCHK(c, mk.mark());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, mk.add(0, c->st.finish_ms));
    // no flipped run: merge_runs_packed takes a single run as it is, but the
    // staying run may hold equal neighbours (k mod 32 in {29, 30, 31})
    if (n_flip == 0) return merge_one_run(c, stay.p, n_stay);
    flip = take_fin_packed(c);
    return merge_runs_packed(c, {{stay.p, n_stay}, {flip.p, nf}});
}

kc_status kc_canonicalize(kc_ctx* c, uint64_t* n_records) {
    if (!c) return KC_ERR_ARG;
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    if (!c->runs.empty()) return fail(c, KC_ERR_STATE, "spill runs exist: write the output and use the file form");
    if (c->count.n_records) {
        HIPCHK(c, hipSetDevice(c->cfg.device));
        DevBuf stay, flip;
        const kc_status s = canon_fold(c, c->count.n_records, stay, flip);
        // retired run buffers join the pool, as after kc_finish's merge
        if (stay.p) c->run_pool.push_back(std::move(stay));
        if (flip.p) c->run_pool.push_back(std::move(flip));
        if (s) return s;
    }
    if (n_records) *n_records = c->count.n_records;
    return KC_OK;
}

// The records counted so far become a sorted run — the reference's sorted
// spill (sortKmers + reduceKMers + FileDump::dumpKmersToFile,
// GPUHandler.cu:456-468, FileDump.cpp:51-58): finished into packed
// SortedKMerFile records (finish_part), kept in HBM outside the counting
// working set (host memory, as a spill run, when HBM is short), and the
// record state starts empty. kc_finish merges the runs on the device.
static kc_status cut_run(kc_ctx* c) {
    kc_status s;
    // inside a flush of padded / one-pass rows: key 0's presence from the reads
    if (c->var_rlen && (s = recompute_presence(c))) return s;
    if ((s = sync_stats(c))) return s;
    uint64_t n = 0;
    const double t0 = kc::trace_on() ? kc::now_s() : 0;
    if ((s = finish_part(c, &n))) return s;  // fin_packed
    HIPCHK(c, hipStreamSynchronize(c->stream));
    kc::trace("cut_run: %llu records finished in %.3f ms", (unsigned long long)n, (kc::now_s() - t0) * 1e3);
    return keep_finished_run(c, n);
}

// fin_packed (n finished records) becomes a sorted run and the record state
// starts empty
kc_status keep_finished_run(kc_ctx* c, uint64_t n) {
    const size_t bytes = (size_t)n * c->rs;
    if (n) {
        // the run takes over fin_packed's buffer
        size_t mfree = 0, mtotal = 0;
        if (!test_hook("KC_HOST_RUNS") && hipMemGetInfo(&mfree, &mtotal) == hipSuccess &&
            mfree > ((size_t)4 << 30)) {
            c->dev_runs.push_back(take_fin_packed(c));
            c->dev_run_n.push_back(n);
            c->count.runs_cut++;
        } else {
            HostRun hr;
            hr.records = n;
            hr.mem.resize(bytes);
            HIPCHK(c, hipMemcpyAsync(hr.mem.data(), c->fin_packed.p, bytes, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            c->runs.push_back(std::move(hr));
        }
    }
    // empty record state: records, batch count, table claims, key 0, descriptors
    c->count.rec_n = 0;
    c->count.batches_cut += c->count.batches;
    c->count.batches = 0;
    c->count.skm_used = false;
    HIPCHK(c, hipMemsetAsync(c->rec_cursor, 0, 8, c->stream));
    if (c->stats_h[ST_CLAIMED]) HIPCHK(c, hipMemsetAsync(c->table, 0, c->table_bytes, c->stream));
    for (int st : {(int)ST_CLAIMED, (int)ST_KEY0, (int)ST_KEY0_PRESENT, (int)ST_DESC_FILL}) c->stats_h[st] = 0;
    HIPCHK(c, hipMemcpyAsync(c->stats, c->stats_h, ST_N * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KC_OK;
}

// A run is cut when the records outgrow half the working set (the reference's
// "table capacity < distinct" case, SURVEY §8d cfg 5).
kc_status cut_run_if_full(kc_ctx* c) {
    const uint64_t M = c->cfg.gpu_memory_limit ? c->cfg.gpu_memory_limit : 100000000ull;
    if (!c->part || c->count.rec_n * (uint64_t)c->rs <= M / 2) return KC_OK;
    return cut_run(c);
}

// The device runs' buffers join the pool
void release_dev_runs(kc_ctx* c) {
    for (auto& r : c->dev_runs) c->run_pool.push_back(std::move(r));
    c->dev_runs.clear();
    c->dev_run_n.clear();
}

kc_status kc_merge_runs_device(kc_ctx* c, const void* d_packed, const uint64_t* run_counts, uint32_t nruns) {
    if (!c || (nruns && !run_counts)) return KC_ERR_ARG;
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    if (!c->runs.empty()) return fail(c, KC_ERR_STATE, "spill runs exist");
    std::vector<std::pair<const void*, uint64_t>> runs;
    uint64_t off = 0;
    for (uint32_t r = 0; r < nruns; r++) {
        runs.push_back({(const uint8_t*)d_packed + off * c->rs, run_counts[r]});
        off += run_counts[r];
    }
    if (off && !d_packed) return KC_ERR_ARG;
    // one run may repeat keys (the SoA path sums them); two or more runs come
    // from finished runs: merged packed, repeated keys summed after the merge
    if (nruns >= 2) return merge_runs_packed(c, runs);
    return merge_one_run(c, d_packed, off);
}

kc_status kc_exchange_contexts(kc_ctx* const* ctxs, uint32_t n) {
    if (!ctxs || n == 0) return KC_ERR_ARG;
    for (uint32_t r = 0; r < n; r++) {
        if (!ctxs[r] || ctxs[r]->W != ctxs[0]->W) return KC_ERR_ARG;
        if (!ctxs[r]->count.finished) return fail(ctxs[r], KC_ERR_STATE, "call kc_finish first");
        if (!ctxs[r]->runs.empty()) return fail(ctxs[r], KC_ERR_STATE, "spill runs exist");
    }
    const uint64_t rs = (uint64_t)ctxs[0]->rs;
    std::vector<std::vector<uint64_t>> cnt(n, std::vector<uint64_t>(n));
    kc_status s;
    for (uint32_t r = 0; r < n; r++)
        if ((s = kc_owner_counts(ctxs[r], n, cnt[r].data()))) return s;
    // Gather every owner's slices before any merge: a merge overwrites the
    // owner's own packed run, which the other owners still read from.
    std::vector<void*> recv(n, nullptr);
    std::vector<uint64_t> m(n, 0);
    auto release = [&]() {
        for (uint32_t o = 0; o < n; o++)
            if (recv[o]) {
                (void)hipSetDevice(ctxs[o]->cfg.device);
                (void)hipFree(recv[o]);
            }
    };
    for (uint32_t o = 0; o < n; o++) {
        kc_ctx* co = ctxs[o];
        for (uint32_t r = 0; r < n; r++) m[o] += cnt[r][o];
        hipError_t e = hipSetDevice(co->cfg.device);
        if (e == hipSuccess) e = hipMalloc(&recv[o], m[o] * rs + 16);
        uint64_t off = 0;
        for (uint32_t r = 0; r < n && e == hipSuccess; r++) {
            uint64_t src = 0;
            for (uint32_t p = 0; p < o; p++) src += cnt[r][p];
            uint64_t bytes = cnt[r][o] * rs;
            if (bytes)
                e = hipMemcpyPeerAsync((uint8_t*)recv[o] + off, co->cfg.device,
                                       (const uint8_t*)ctxs[r]->fin_packed.p + src * rs, ctxs[r]->cfg.device, bytes,
                                       co->stream);
            off += bytes;
        }
        if (e != hipSuccess) {
            release();
            return fail(co, KC_ERR_HIP, hipGetErrorString(e));
        }
    }
    for (uint32_t o = 0; o < n; o++) {
        hipError_t e = hipSetDevice(ctxs[o]->cfg.device);
        if (e == hipSuccess) e = hipStreamSynchronize(ctxs[o]->stream);
        if (e != hipSuccess) {
            release();
            return fail(ctxs[o], KC_ERR_HIP, hipGetErrorString(e));
        }
    }
    // owner o received one sorted slice from every context, in order; the
    // owners merge concurrently, one host thread each (each context has its
    // own stream and buffers; hipSetDevice is per thread)
    std::vector<kc_status> ms(n, KC_OK);
    auto merge_owner = [&](uint32_t o) {
        std::vector<uint64_t> rc(n);
        for (uint32_t r = 0; r < n; r++) rc[r] = cnt[r][o];
        if (hipSetDevice(ctxs[o]->cfg.device) != hipSuccess) {
            ms[o] = fail(ctxs[o], KC_ERR_HIP, "hipSetDevice(%d)", ctxs[o]->cfg.device);
            return;
        }
        ms[o] = kc_merge_runs_device(ctxs[o], recv[o], rc.data(), n);
    };
    if (n == 1) {
        merge_owner(0);
    } else {
        std::vector<std::thread> th;
        for (uint32_t o = 0; o < n; o++) th.emplace_back(merge_owner, o);
        for (auto& t : th) t.join();
    }
    release();
    for (uint32_t o = 0; o < n; o++)
        if (ms[o]) return ms[o];
    return KC_OK;
}

kc_status kc_gather_contexts(kc_ctx* const* ctxs, uint32_t n) {
    if (!ctxs || n == 0) return KC_ERR_ARG;
    for (uint32_t r = 0; r < n; r++) {
        if (!ctxs[r] || ctxs[r]->W != ctxs[0]->W) return KC_ERR_ARG;
        if (!ctxs[r]->count.finished) return fail(ctxs[r], KC_ERR_STATE, "call kc_finish first");
        if (!ctxs[r]->runs.empty()) return fail(ctxs[r], KC_ERR_STATE, "host spill runs exist: merge on the host");
    }
    kc_ctx* c0 = ctxs[0];
    const uint64_t rs = (uint64_t)c0->rs;
    uint64_t total = 0;
    for (uint32_t r = 0; r < n; r++) total += ctxs[r]->count.n_records;
    HIPCHK(c0, hipSetDevice(c0->cfg.device));
    void* recv = nullptr;
    HIPCHK(c0, hipMalloc(&recv, total * rs + 16));
    std::vector<std::pair<const void*, uint64_t>> runs;
    uint64_t off = 0;
    for (uint32_t r = 0; r < n; r++) {
        const uint64_t bytes = ctxs[r]->count.n_records * rs;
        hipError_t e = bytes ? hipMemcpyPeerAsync((uint8_t*)recv + off * rs, c0->cfg.device, ctxs[r]->fin_packed.p,
                                                  ctxs[r]->cfg.device, bytes, c0->stream)
                             : hipSuccess;
        if (e != hipSuccess) {
            (void)hipFree(recv);
            return fail(c0, KC_ERR_HIP, "gather: %s", hipGetErrorString(e));
        }
        runs.push_back({(uint8_t*)recv + off * rs, ctxs[r]->count.n_records});
        off += ctxs[r]->count.n_records;
    }
    hipError_t e = hipStreamSynchronize(c0->stream);
    kc_status s = e == hipSuccess ? merge_runs_packed(c0, runs) : fail(c0, KC_ERR_HIP, "gather: %s", hipGetErrorString(e));
    (void)hipFree(recv);
    return s;
}
