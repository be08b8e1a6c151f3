// kc_ctx.h — internal to libkc_hip: the device context behind include/kc.h's
// kc_ctx, the buffers it owns, and the host functions that cross between the
// library's stage files (kc_api.cpp, kc_count.cpp, kc_ingest.cpp, kc_finish.cpp). No part of the
// library's interface.
#pragma once
#include <hip/hip_runtime_api.h>

#include <string>
#include <vector>

#include "../../include/kc.h"
#include "kc_device.h"
#include "kc_stage.h"

using namespace kc;

#pragma GCC visibility push(hidden)

// A device allocation that frees itself. Move-only: a buffer changes hands by
// std::move or std::swap, and a moved-from DevBuf is empty.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
        o.p = nullptr;
        o.bytes = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            std::swap(p, o.p);
            std::swap(bytes, o.bytes);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // Replaces the allocation by one of exactly n bytes (contents undefined).
    hipError_t alloc(size_t n) {
        release();
        const hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        else p = nullptr;
        return e;
    }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

// A DevBuf of T that stands where a T* does (launch arguments, pointer
// arithmetic, null tests). The pointer it converts to is borrowed: it is good
// until the owner is reallocated, swapped or moved from (grow_records swaps
// rec_keys, rec_cnts and rec_dig), so take it where it is used and keep no
// T* copy of a member across a call that may grow it.
template <class T>
struct DevArr : DevBuf {
    operator T*() const { return as<T>(); }
};

struct HostRun {
    std::vector<uint8_t> mem;  // used when no temp dir
    std::string path;          // used with a temp dir
    uint64_t records = 0;
};

#pragma GCC visibility pop

// The host-side counters one batch adds to (kc_stats timings and launch
// counts, engine flags): copied before a batch that may be undone.
struct BatchCounters {
    uint64_t insert_launches = 0;  // kc_stats.insert_launches, insert_ms
    double insert_ms = 0;
    double part_ms[5] = {0, 0, 0, 0, 0};  // E+P1, P2, P3 scatter, P3 hist + P4, P5
    double dedup_ms = 0;                  // skm P5a
    uint64_t p5_launches = 0;
    uint64_t part_keys = 0;     // keys partitioned since the last reset
    bool skm_used = false;      // a batch went through the skm engine since the last reset
    bool skm_checked = false;   // the skm cardinality sample has run since the last reset
    uint32_t engines_used = 0;  // kc_stats.engines_used
};

// The state of one count: everything kc_reset returns to its initial value,
// which is the value written here.
struct CountState : BatchCounters {
    uint64_t rec_n = 0;  // records, host copy after each batch
    uint64_t batches = 0;
    double presplit_ms = 0;  // P3b (also in part_ms[2])
    uint64_t presplit_batches = 0, sorted_run_batches = 0, key_passes = 0;
    double finish_group_ms = 0;  // the finish's grouping passes (histograms + scatters)
    uint64_t dedup_records = 0;
    bool skm_big_off = false;  // a large skm batch overflowed the spill or record buffer: safe batches only
    bool skm_hc = false;       // high cardinality seen: the key-prefix engine counts
    bool hc_hint = false;      // most keys were distinct (the skm sample or the last key-prefix batch):
                               // P5 splits buckets by their key count up front
    uint64_t spilled_flushed = 0;
    uint64_t runs_cut = 0;
    uint64_t batches_cut = 0;  // batches of the records already cut into runs
    // the pending batch (see kc_ctx, "Pending batch")
    int64_t pend_L = 0;
    bool pend_var = false;
    uint64_t pend_reads = 0;
    bool pend_sparse = false;
    size_t acc_n = 0;   // bytes in the kc_count_chunk accumulation buffer (kc_ctx::acc_buf)
    bool ckpt = false;  // a checkpoint is held (kc_ctx::ckpt_*)
    // results
    bool finished = false;
    uint64_t n_records = 0;  // table run
};

// kc_ctx (kc.h declares it) and Marks stay visible; -Wattributes remarks on the hidden field types
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wattributes"
struct kc_ctx {
    kc_config cfg;
    std::string temp_dir;
    int W = 1, rs = 12;
    int64_t k = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev2 = nullptr;  // a third mark: two phases timed by one synchronisation
    hipEvent_t evf[2] = {nullptr, nullptr};  // kc_finish's own marks (the passes inside it use ev0..ev2)
    uint64_t id = 0;
    CountState count;

    // table + spill (the gpu_memory_limit working set)
    DevArr<uint64_t> table;
    uint64_t cap = 0;
    size_t table_bytes = 0;
    bool table_dirty = true;  // a slot may be non-zero (cleared by kc_reset)
    DevArr<uint64_t> spill;
    uint64_t spill_cap = 0;
    DevArr<uint64_t> stats;         // device ST_N
    uint64_t* stats_h = nullptr;    // pinned host mirror

    // partition engine (default): key buffers for one batch, records
    bool part = true;
    bool skm = false;              // KC_FLAG_ENGINE_SKM: super-k-mer records instead of keys
    bool skm_force = false;        // KC_FLAG_ENGINE_SKM: no cardinality sample
    DevArr<uint64_t> pool_cursor;  // device u64: skm pool allocator
    uint64_t key_cap = 0;          // keys per batch
    DevArr<uint64_t> keys_a;       // W x key_cap
    DevArr<uint8_t> digs;          // digs_bytes: P3 digit (word0 >> 56) of keys_a[i], written by P2; the skm
                                   // engine keeps two digit bytes per record (both grouping passes)
    uint64_t digs_bytes = 0;
    DevArr<uint64_t> keys_b;
    DevBuf part_hist, part_base, part_tmp, part_starts, part_sort_hist;
    DevBuf part_ghist;  // key-range passes: P1 histogram by 16 key groups (+ the group totals)
    DevBuf part_base2;  // key-range passes: the second pass of a walk's run starts
    DevBuf part_dedup;  // skm P5a: per-bucket list starts (u64) and lengths (u32), list cursor
    DevBuf p3b_buf, sub_starts;  // key-prefix engine, high cardinality: P3b tile positions, sub-bucket starts
    DevBuf run_flags;            //   P5s: runs left to the LDS hash path
    DevBuf part_codes, part_inval;  // kernel E output: the batch's reads, 2-bit encoded
    DevBuf part_rlen;               // KC_FLAG_VARLEN: each read's own length (u16)
    const uint16_t* var_rlen = nullptr;  // set while a variable-length block is counted
    // P5 segment descriptors (see finish_part_sorted) and their sort scratch
    DevBuf desc_key, desc_start, desc_len, desc_k2, desc_v, desc_v2, desc_lens, desc_offs, desc_fb;
    DevArr<uint64_t> rec_keys;     // W x rec_cap
    DevArr<uint8_t> rec_dig;       // rec_cap: word 0 bits 48..55 of each record the skm P5 wrote (the
                                   // finish's first grouping digit, read as 1 B instead of word 0)
    DevArr<uint32_t> rec_cnts;
    uint64_t rec_cap = 0;
    DevArr<uint64_t> rec_cursor;  // device u64
    int n_cu = 256;

    // scratch (grown on demand)
    DevBuf in_stage;        // host-pointer inputs
    DevBuf fq_counts, fq_base, fq_tmp, seq_off, seq_end;
    DevBuf fq_phase;  // one-pass index: each chunk's guessed line phase
    DevBuf spill_keys2, rle_flags, rle_pos, rle_head, rle_tmp, run_keys, run_cnts, run_packed;
    DevBuf fin_keys[2], fin_cnts[2], fin_hist, fin_packed, fin_misc;
    DevBuf merge_tmp;  // packed run merge: the other ping-pong buffer
    DevBuf q_bins, q_tiles, q_keys, q_counts, q_found;  // queries on the finished run: histogram bins (+ the
                                                        // lookup's found counter), filter tile counts /
                                                        // bases / scan scratch, kc_lookup's staged arrays

    // host staging (kc_stage.h), created on the first host-pointer input or output
    kc::Pool* pool = nullptr;
    kc::PinnedRing* ring = nullptr;
    std::vector<char*> file_bufs;  // pinned blocks of kc_count_file's reader (kept: pinning is slow)
    size_t file_buf_bytes = 0;
    hipStream_t copy_stream = nullptr;  // kc_count_file: block i+1 uploads while block i is decoded
    hipEvent_t file_ev[2] = {nullptr, nullptr};
#pragma GCC diagnostic pop
    hipEvent_t stage_free[2] = {nullptr, nullptr};  // kc_count_chunk: the encode of the staged chunk is done
    DevBuf file_stage[2];
    int chunk_slot = 0;
    // kc_count_chunk accumulation: whole reads of consecutive chunks copied
    // into one of two pinned buffers, uploaded and encoded when it fills (or
    // before anything else counts, finishes or checkpoints)
    char* acc_buf[2] = {nullptr, nullptr};
    hipEvent_t acc_ev[2] = {nullptr, nullptr};
    bool acc_busy[2] = {false, false};
    int acc_i = 0;
    int64_t acc_L = 0;
    double acc_t[4] = {0, 0, 0, 0};  // KC_TRACE: host copy, buffer wait, flush, calls (s)

    // Pending batch: reads already indexed and 2-bit encoded into part_codes /
    // part_inval (/ part_rlen) by kc_count_* calls, counted together at the
    // next flush (when the next block does not fit, its read length differs,
    // or at kc_finish). Many small calls thus count as one batch
    // (count.pend_L, pend_var, pend_reads). count.pend_sparse:
    // the pending rows hold one-pass-indexed blocks (rows per chunk, empty rows
    // of length 0): every pending row has its length in part_rlen, the skm
    // front end reads them, and key 0's presence is recomputed at the flush
    // from ST_VHOLE as for variable-length reads
    uint64_t flush_present0 = 0;  // key 0's presence before the flush of padded / one-pass rows
    uint64_t flushes = 0;
    uint64_t dev_total = 0;  // device memory (bytes)
    // kc_checkpoint / kc_rollback: the pending state and the counters a
    // rolled-back block may have changed (held: count.ckpt)
    uint64_t ckpt_reads = 0, ckpt_flushes = 0, ckpt_st_reads = 0, ckpt_st_windows = 0;
    uint64_t ckpt_stats[ST_N];

    // Sorted runs cut from the records when they outgrow half the working set
    // (cut_run): kept in HBM outside the counting working set (host memory
    // only when HBM is short, as c->runs), merged on the device by kc_finish
    std::vector<DevBuf> dev_runs;
    std::vector<uint64_t> dev_run_n;
    std::vector<DevBuf> run_pool;  // run buffers of earlier counts, reused (allocations are kept like all others)

    std::vector<HostRun> runs;  // spill runs in host memory or temp files

    kc_stats st;
    std::string err;
};

// Timing marks on the stream (ev0..ev2). begin() records mark 0 (or restarts
// at mark `at`), mark() the next one. The wait stays with the caller, whose
// kind of wait varies and often carries a copy as well; after it, ms(i) is the
// time from mark i to mark i + 1, and add(i, slots...) adds it to counters.
struct Marks {
    kc_ctx* c;
    int n = 0;
    hipEvent_t ev(int i) const { return i == 0 ? c->ev0 : i == 1 ? c->ev1 : c->ev2; }
    hipError_t begin(int at = 0) {
        n = at;
        return mark();
    }
    hipError_t mark() { return hipEventRecord(ev(n++), c->stream); }
    hipEvent_t last() const { return ev(n - 1); }
    hipError_t ms(int i, float* t) const { return hipEventElapsedTime(t, ev(i), ev(i + 1)); }
    template <class... Slot>
    hipError_t add(int i, Slot&... slot) const {
        float t = 0.f;
        const hipError_t e = ms(i, &t);
        if (e == hipSuccess) ((slot += t), ...);
        return e;
    }
};

#pragma GCC visibility push(hidden)

kc_status fail(kc_ctx* c, kc_status s, const char* fmt, ...);

#define HIPCHK(ctx, expr)                                                                                    \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return fail((ctx), e_ == hipErrorOutOfMemory ? KC_ERR_NOMEM : KC_ERR_HIP, "%s: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                          \
    } while (0)

// KC_DEBUG: "kc:" lines on stderr. Read at every use: a caller may set it
// between two calls of a live process.
inline bool debug_on() { return getenv("KC_DEBUG") != nullptr; }

static const int kBucketBits = 16;
static const uint64_t kDescCap = 1u << 20;  // P5 segment descriptors kept for the sorted finish

// helpers of every stage (kc_api.cpp)
kc_status ensure(kc_ctx* c, DevBuf& b, size_t bytes);
kc_status ensure_pooled(kc_ctx* c, DevBuf& b, size_t bytes);
DevBuf take_fin_packed(kc_ctx* c);
kc_status sync_stats(kc_ctx* c);

// counting (kc_count.cpp): towards ingest, the engine choice and the calls
// that count reads ...
enum class Engine { skm, prefix, table };  // super-k-mer, key-prefix ("partition"), global table
Engine engine_for(const kc_ctx* c, int64_t L);
uint64_t batch_reads(const kc_ctx* c, int64_t L);
CountLaunch make_launch(const kc_ctx* c, const uint8_t* base, const uint64_t* seq_off, uint64_t read0, uint64_t nr,
                        int64_t L, int64_t pre0);
kc_status count_reads(kc_ctx* c, const uint8_t* base, const uint64_t* seq_off, uint64_t n_reads, int64_t L,
                      int64_t pre0 = -1);
kc_status count_pending_fixed(kc_ctx* c, uint64_t n, int64_t L);
// ... and towards the finish, the record buffer and the 16-bit grouping
kc_status grow_records(kc_ctx* c, uint64_t need);
kc_status group16(kc_ctx* c, int NW, bool pay, uint64_t* a, uint64_t sa, uint32_t* pa, uint64_t* b, uint64_t sb,
                  uint32_t* pb, uint8_t* digs, uint64_t n, double* ms, const uint8_t* dig1 = nullptr);
RecSink rec_sink(const kc_ctx* c);
DescSink desc_sink(const kc_ctx* c);

// ingest (kc_ingest.cpp), used by counting, the finish and the output
kc_status recompute_presence(kc_ctx* c);
kc_status pend_flush(kc_ctx* c);
kc_status stage_init(kc_ctx* c);

// finish and run merging (kc_finish.cpp), used by counting and the lifecycle
kc_status sort_records(kc_ctx* c, uint64_t* ka, uint64_t* kb, uint32_t* va, uint32_t* vb, uint64_t stride, uint64_t n,
                       int* which, int words = 0);
kc_status flush_spill(kc_ctx* c);
kc_status flush_spill2(kc_ctx* c, uint64_t* spill, uint64_t* scratch);
kc_status cut_run_if_full(kc_ctx* c);
kc_status keep_finished_run(kc_ctx* c, uint64_t n);
void release_dev_runs(kc_ctx* c);

#pragma GCC visibility pop
