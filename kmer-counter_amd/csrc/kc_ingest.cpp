// kc_ingest.cpp — ingest: the pending batch and everything that feeds it. The
// FASTQ index (ingest_fastq), the chunk and FASTQ entry points with their
// staged uploads, the file reader (kc_count_file), and checkpoint / rollback of
// the pending state. The engines it feeds are in kc_count.cpp.
#include <errno.h>
#include <sched.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <thread>

#include "kc_ctx.h"
#include "kc_io.h"

static kc_status check_line(kc_ctx* c, int64_t L) {
    if (L < c->k) return fail(c, KC_ERR_ARG, "read length %lld is shorter than k=%lld", (long long)L, (long long)c->k);
    if (L > 32767) return fail(c, KC_ERR_ARG, "read length %lld exceeds 32767 (the reference's u16 2L header)",
                               (long long)L);
    return KC_OK;
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

static kc_status chunk_acc_flush(kc_ctx* c);  // (with the chunk entry points: its chunk_device flushes in turn)

// Counts the pending batch (the engines: count_reads with pre-encoded reads).
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
    if (!c->count.pend_var && !sparse) return count_pending_fixed(c, n, c->count.pend_L);
    // variable-length reads (slot padding) or one-pass rows (empty rows): the
    // skm front end reads each row's length; key 0's presence is recomputed
    kc_status s;
    if ((s = sync_stats(c))) return s;
    c->flush_present0 = c->stats_h[ST_KEY0_PRESENT];
    c->var_rlen = c->part_rlen.as<uint16_t>();
    s = c->count.pend_var ? count_reads(c, nullptr, nullptr, n, c->count.pend_L, 0)
                          : count_pending_fixed(c, n, c->count.pend_L);
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
    const Engine engine = engine_for(c, L);
    const bool f3_rows = engine == Engine::skm && c->W == 1 && c->k >= 19 && c->k <= 32 &&
                         skm_f3_applies((int)L, (int)c->k);
    const bool spec = count && !var && !two_pass && !no_spec && f3_rows && fq_spec_ok((int)L) &&
                      !test_hook("KC_NO_FQ_ENCODE") && !test_hook("KC_NO_FQ_SPEC");
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
    const bool codes = engine != Engine::table;  // (2-bit codes; the table engine reads the text)
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

// Host staging (pinned ring + copy pool), created on first use.
kc_status stage_init(kc_ctx* c) {
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
    if (engine_for(c, L) != Engine::table) {
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

// Uploads host bytes into staging buffer `slot` on the copy stream: through the
// pinned ring (pageable source) or straight from a pinned buffer (src_done,
// when given, is recorded once it has been read). The upload waits for
// stage_free[slot], which the last reader of the buffer recorded on the ctx
// stream; the next reader waits for file_ev[slot] there.
static kc_status stage_upload(kc_ctx* c, int slot, const char* src, size_t bytes, bool pinned_src,
                              hipEvent_t src_done) {
    kc_status s;
    if ((s = copy_stream_init(c))) return s;
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
    return KC_OK;
}

// One staged upload + encode of host bytes (whole reads of length L) into one
// of the two staging buffers in turn; the encode waits for that upload on the
// ctx stream, so the next upload overlaps this encode.
static kc_status chunk_upload_count(kc_ctx* c, const char* src, size_t bytes, int64_t L, bool pinned_src,
                                    hipEvent_t src_done, bool add_stats) {
    kc_status s;
    const int slot = c->chunk_slot;
    c->chunk_slot ^= 1;
    if ((s = stage_upload(c, slot, src, bytes, pinned_src, src_done))) return s;
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->file_ev[slot], 0));
    if ((s = chunk_device(c, (const uint8_t*)c->file_stage[slot].p, (int64_t)bytes, L, add_stats))) return s;
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
        // (the reader's blocks are pinned; it refills one when its decode returns, so no source event)
        kc_status s = have ? stage_upload(c, slot, cur.p, cur.n, true, nullptr) : KC_OK;
        while (have && !s) {
            const bool have_nxt = !stop && rd.next(&nxt);
            if (have_nxt && (s = stage_upload(c, slot ^ 1, nxt.p, nxt.n, true, nullptr))) {
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

kc_status kc_count_file(kc_ctx* const* ctxs, uint32_t n_ctx, const char* path, int64_t L, uint32_t mode,
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
